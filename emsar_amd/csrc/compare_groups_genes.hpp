// compare_groups_genes.hpp -- the gene-level K-sample test across replicate groups behind include/emsar_hip.h:
// emsar_hip_compare_groups_genes.  Part of emsar_hip.hip's translation unit, included after compare_groups.hpp (GroupsLayout,
// groups_reduce, groups_host_searches) and gene_parts.hpp: the members of the queried genes are located in every sample as the
// two-sample gene test locates them (SetQuery, GeneQueryMembers, GenePartLists), k_compare_groups_gene_sets
// (kernels_compare_groups_genes.hpp) runs the searches.
// One call = one GroupsGenesRun:  plan, classify   SetQuery's stages on the union of the queried genes' members, once per context
//                                 place            per gene and sample: the members taking part by part, the smallest den; the host-only
//                                                  statuses; a gene whose parts are all closed form in every sample is searched on the
//                                                  host; any other gets one item for all samples and one per group of two or more (a
//                                                  single group IS all samples: one item), each in the launch class of the largest set
//                                                  part among its samples; the locator table [gene][K], the sample table [K] and the
//                                                  part lists go to the device
//                                 search           the items in batches across the three launch classes (SetItemRunner)
//                                 reduce           records -> the two Lambdas, p, the common values, status (groups_reduce);  copy_out in
//                                                  query order
// One workgroup runs one two-level search.  No context's theta, weights or scales are touched.  The launches run on the first context's
// streams; the others' streams are drained before.

namespace {

enum { GRP_TOO_LARGE = EMSAR_GENE_GROUPS_TOO_LARGE };

// The closed-form parts of a gene in K samples as groups_search's samples: gene_closed_sum as the evaluation, mn[k] as den
struct GroupGeneClosedSamples {
    const CompareGeneClosed *const *closed;        // [K] sample k's list
    const int *n;                        // [K]
    const double *mn, *size_;            // [K]
    double th[kGroupsMax], Fh[kGroupsMax];
    double size(int k) const { return size_[k]; }
    double den(int k) const { return mn[k]; }
    double hat(int k) const { return th[k]; }
    void put_hat(int k, double x, double F) { th[k] = x; Fh[k] = F; }
    void eval(int k, double scale, double lambda, double &x, double &F) const {
        GeneSums S{0.0, 0.0, 0.0};
        gene_closed_sum(closed[k], n[k], GenePoint{mn[k], scale, lambda, -1, 0.0}, S);
        x = S.X; F = S.F;
    }
};
// The searches of k_compare_groups_gene_sets on a gene whose parts are all closed form in every sample, and their reduction: what the
// host does for such genes
inline bool groups_closed_gene(const GroupsLayout &L, const CompareGeneClosed *const *closed, const int *n, const double *mn,
                               const GroupSearchParams &Q, GroupsResult &o, double *gene_group, double *gene_hat) {
    return groups_host_searches(L, GroupGeneClosedSamples{closed, n, mn, L.size.data(), {}, {}}, Q, o, gene_group, gene_hat);
}

struct GroupsGenesRun : GeneQueryMembers {
    struct Result : GroupsResult { int32_t parts = 0; };       // per queried gene; theta_common holds the common gene sum
    emsar_hip_ctx *const ctx;            // the first sample's: its gene map, its streams and events
    emsar_hip_ctx *const *const ctxs;    // [K]
    GroupsLayout L;
    const emsar_em_params *const p;      // the caller's solver parameters (SetQuery fills in the defaults)
    const int32_t nq;
    const int32_t *const query;          // gene ids, null = all in order
    const emsar_groups_gene_outputs out; // a copy: all NULL when the caller gave none
    const GroupSearchParams Q;
    std::vector<std::unique_ptr<SetQuery>> q;      // [K] where every member stands in each sample
    std::vector<Result> res;             // per gene slot
    std::vector<double> res_group, res_hat;        // [slot][G], [slot][K]
    GenePartLists lists;
    std::vector<DevBuf<int32_t>> d_gene_of;        // [K] context k's gene_of_lib when it has no map of its own
    SetItemRunner<GroupGeneItem, GroupRec> runner;
    emsar_groups_gene_stats st{};

    GroupsGenesRun(emsar_hip_ctx *c0, emsar_hip_ctx *const *cs, const GroupsLayout &lay, const emsar_em_params *pp, const emsar_groups_params &gp,
                   int32_t nq_, const int32_t *query_, const emsar_groups_gene_outputs *o)
        : ctx(c0), ctxs(cs), L(lay), p(pp), nq(nq_), query(query_), out(o ? *o : emsar_groups_gene_outputs{}), Q(groups_search_params(gp)),
          d_gene_of((size_t)lay.K), runner(c0, "EMSAR_HIP_GROUPS_GENES_BATCH", "compare_groups_genes: an item lies outside its class's sets") {
        st.df_between = L.G - 1; st.df_within = L.K - L.G;
    }

    int32_t gene_of_query(int32_t i) const { return query ? query[i] : i; }
    int fail_numeric() { ctx->err = "compare_groups_genes: non-finite likelihood at lambda = 0"; return EMSAR_HIP_ERR_NUMERIC; }
    void note_raw(const Result &o) {
        if (o.raw_between < st.min_raw_lambda) st.min_raw_lambda = o.raw_between;
        if (o.raw_within < st.min_raw_lambda) st.min_raw_lambda = o.raw_within;
    }

    int place_search_reduce() {
        const int K = L.K, G = L.G;
        const size_t n_slots = genes.size();
        res.resize(n_slots);
        res_group.assign(n_slots * (size_t)G, NAN); res_hat.assign(n_slots * (size_t)K, NAN);
        std::vector<GroupGeneLoc> locs(n_slots * (size_t)K, GroupGeneLoc{0, 0, 0, 0, 0.0});
        std::vector<GroupGeneItem> items[emsar::kSetClasses];
        std::vector<GroupRec> recs[emsar::kSetClasses];
        struct Where { int32_t cls = -1, idx = -1; };
        std::vector<Where> where(n_slots * (size_t)(G + 1));   // [slot][0] the all-samples item, [slot][1 + g] group g's
        std::vector<int32_t> row_of(n_slots, -1);
        int32_t n_rows = 0;
        bool resident = true;
        for (int k = 0; k < K; k++) resident = resident && q[(size_t)k]->use_sets;
        std::vector<GeneSideParts> sides((size_t)K);
        std::vector<const GeneSideParts *> side_ptr((size_t)K);
        for (size_t i = 0; i < n_slots; i++) {
            Result &o = res[i];
            if (!resident) { o.status = GRP_NOT_RESIDENT; continue; }
            bool away = false, outside = false, large = false, closed = true;
            int32_t n_parts = 0;
            for (int k = 0; k < K; k++) {
                sides[(size_t)k] = side_parts(*q[(size_t)k], i, k);
                side_ptr[(size_t)k] = &sides[(size_t)k];
                const GeneSideParts &s = sides[(size_t)k];
                away = away || s.not_resident;
                outside = outside || s.count() == 0;
                large = large || s.count() > kGeneMaxParts;
                closed = closed && s.sets.empty();
                n_parts += s.count();
            }
            if (away) { o.status = GRP_NOT_RESIDENT; continue; }
            if (outside) { o.status = GRP_OUTSIDE; continue; }
            if (large) { o.status = GRP_TOO_LARGE; continue; }
            o.parts = n_parts;
            st.parts_max = std::max(st.parts_max, o.parts);
            if (closed) {
                const CompareGeneClosed *cl[kGroupsMax];
                int n[kGroupsMax];
                double mn[kGroupsMax];
                for (int k = 0; k < K; k++) { cl[k] = sides[(size_t)k].closed.data(); n[k] = (int)sides[(size_t)k].closed.size(); mn[k] = sides[(size_t)k].min_den; }
                if (!groups_closed_gene(L, cl, n, mn, Q, o, &res_group[i * (size_t)G], &res_hat[i * (size_t)K])) return fail_numeric();
                note_raw(o);
                continue;
            }
            GenePartLists::Offsets at = lists.append(side_ptr.data(), K);
            GroupGeneLoc *row = &locs[i * (size_t)K];
            for (int k = 0; k < K; k++) {
                const GeneSideParts &s = sides[(size_t)k];
                row[k] = GroupGeneLoc{at.part_off, (int32_t)s.sets.size(), at.closed_off, (int32_t)s.closed.size(), s.min_den};
                at.part_off += (int32_t)s.sets.size(); at.closed_off += (int32_t)s.closed.size();
            }
            const auto add = [&](uint32_t mask, int32_t row_id, Where &w) {
                int cls = 0;                                                     // no set part in any sample of the subset: the smallest launch
                for (int k = 0; k < K; k++) if ((mask >> k) & 1u) cls = std::max(cls, lists.launch_class(row[k].part_off, row[k].n_parts));
                w.cls = cls; w.idx = (int32_t)items[cls].size();
                items[cls].push_back(GroupGeneItem{(int32_t)i, row_id, mask, genes[i]});
            };
            row_of[i] = n_rows++;
            add(L.all, row_of[i], where[i * (size_t)(G + 1)]);
            for (int g = 0; g < G; g++)
                if (L.mask[(size_t)g] != L.all && GroupsLayout::count(L.mask[(size_t)g]) >= 2) add(L.mask[(size_t)g], -1, where[i * (size_t)(G + 1) + 1 + (size_t)g]);
        }
        std::vector<double> h_X((size_t)n_rows * (size_t)K), h_F((size_t)n_rows * (size_t)K);
        if (n_rows > 0) {
            std::vector<GroupGeneSample> samples((size_t)K);
            for (int k = 0; k < K; k++) {
                const int32_t *gene_of = nullptr;
                if (const int rc = gene_of_lib_of(ctx, ctxs[k], d_gene_of[(size_t)k], gene_of)) return rc;
                samples[(size_t)k] = GroupGeneSample{side_of(ctxs[k]), L.size[(size_t)k], gene_of};
            }
            if (const int rc = lists.upload(ctx)) return rc;
            DevBuf<GroupGeneSample> d_samples;
            DevBuf<GroupGeneLoc> d_locs;
            DevBuf<double> d_X, d_F;
            HIPCHK(d_samples.upload(samples.data(), samples.size()));
            HIPCHK(d_locs.upload(locs.data(), locs.size()));
            HIPCHK(d_X.alloc(h_X.size())); HIPCHK(d_F.alloc(h_F.size()));
            // the LDS of a launch class: the largest set of that class or a smaller one in any sample, then X_hat^k, K doubles
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
                if (!items[c].empty() && lds[c] > (size_t)lds_limit) { ctx->err = "compare_groups_genes: a launch needs more LDS than the device has"; return EMSAR_HIP_ERR_HIP; }
                HIPCHK(hipFuncSetAttribute((const void *)kCompareGroupsGeneSets[c], hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)(emsar::kSetLdsCap[c] + 8 + kGroupsMax * sizeof(double))));
            }
            const SetSolveParams P = set_params(q[0]->p);
            std::vector<GenePartLists::Side> item_sides((size_t)K);
            const int rc = runner.run(items, recs, st.device_ms, st.items_launched,
                [&](int c, const GroupGeneItem &it) {
                    if (it.q < 0 || (size_t)it.q >= n_slots || it.row < -1 || it.row >= n_rows || (it.mask & ~L.all) || GroupsLayout::count(it.mask) < 2) return false;
                    const GroupGeneLoc *row = &locs[(size_t)it.q * (size_t)K];
                    int32_t part_off = row[0].part_off, closed_off = row[0].closed_off;
                    for (int k = 0; k < K; k++) {                                // the K slices stand one behind the other
                        if (row[k].part_off != part_off || row[k].closed_off != closed_off || row[k].n_parts < 0 || row[k].n_closed < 0) return false;
                        if (!(row[k].min_den > 0.0) || row[k].n_parts + row[k].n_closed < 1) return false;
                        item_sides[(size_t)k] = GenePartLists::Side{ctxs[k], row[k].n_parts, row[k].n_closed};
                        part_off += row[k].n_parts; closed_off += row[k].n_closed;
                    }
                    const int top = lists.slice_class(row[0].part_off, row[0].closed_off, it.gene, item_sides.data(), K, it.mask);
                    return top >= -1 && std::max(top, 0) == c;
                },
                [&](int c, int threads, hipStream_t s, size_t cnt, const GroupGeneItem *d_items, GroupRec *d_rec) {
                    hipLaunchKernelGGL(kCompareGroupsGeneSets[c], dim3((unsigned)cnt), dim3(threads), lds[c], s, d_items, d_samples.get(), d_locs.get(),
                                       lists.d_parts.get(), lists.d_closed.get(), d_X.get(), d_F.get(), d_rec, K, hat_off[c], P, Q);
                });
            if (rc) return rc;
            HIPCHK(hipMemcpy(h_X.data(), d_X, h_X.size() * sizeof(double), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(h_F.data(), d_F, h_F.size() * sizeof(double), hipMemcpyDeviceToHost));
        }
        for (int cls = 0; cls < emsar::kSetClasses; cls++)
            for (const GroupRec &r : recs[cls]) {
                add_search_stats(st, r);
                st.outer_sum += r.outer; st.outer_max = std::max(st.outer_max, r.outer);
            }
        std::vector<const GroupRec *> group((size_t)G);
        for (size_t i = 0; i < n_slots; i++) {
            if (row_of[i] < 0) continue;
            const Where *w = &where[i * (size_t)(G + 1)];
            const GroupRec &all = recs[w[0].cls][(size_t)w[0].idx];
            for (int g = 0; g < G; g++)
                group[(size_t)g] = L.mask[(size_t)g] == L.all ? &all : w[1 + g].cls < 0 ? nullptr : &recs[w[1 + g].cls][(size_t)w[1 + g].idx];
            const double *Xh = &h_X[(size_t)row_of[i] * (size_t)K], *Fh = &h_F[(size_t)row_of[i] * (size_t)K];
            if (!groups_reduce(L, all, group.data(), Xh, Fh, res[i], &res_group[i * (size_t)G])) return fail_numeric();
            std::copy(Xh, Xh + K, &res_hat[i * (size_t)K]);
            note_raw(res[i]);
        }
        return EMSAR_HIP_OK;
    }

    int copy_out() {
        const size_t K = (size_t)L.K, G = (size_t)L.G;
        for (const Result &o : res) st.n_status[o.status]++;
        for (int32_t i = 0; i < nq; i++) {
            const size_t c = (size_t)slot_of_gene[(size_t)gene_of_query(i)];
            const Result &o = res[c];
            if (out.lambda_between) out.lambda_between[i] = o.lambda_between;
            if (out.p_between) out.p_between[i] = groups_pvalue(o.lambda_between, st.df_between);
            if (out.lambda_within) out.lambda_within[i] = o.lambda_within;
            if (out.p_within) out.p_within[i] = groups_pvalue(o.lambda_within, st.df_within);
            if (out.raw_between) out.raw_between[i] = o.raw_between;
            if (out.raw_within) out.raw_within[i] = o.raw_within;
            if (out.gene_common) out.gene_common[i] = o.theta_common;
            if (out.slope) out.slope[i] = o.slope;
            if (out.gene_group) std::copy(&res_group[c * G], &res_group[c * G] + G, out.gene_group + (size_t)i * G);
            if (out.gene_hat) std::copy(&res_hat[c * K], &res_hat[c * K] + K, out.gene_hat + (size_t)i * K);
            if (out.status) out.status[i] = o.status;
            if (out.outer) out.outer[i] = o.outer;
            if (out.evals) out.evals[i] = o.evals;
            if (out.parts) out.parts[i] = o.parts;
        }
        return EMSAR_HIP_OK;
    }

    int run() {
        list_members(ctx->genes, nq, query);
        for (int k = 0; k < L.K; k++) {
            q.emplace_back(new SetQuery(ctxs[k], p, (int32_t)member_tids.size(), member_tids.data()));
            int rc;
            if ((rc = q[(size_t)k]->plan()) || (rc = q[(size_t)k]->classify())) { if (k) ctx->err = ctxs[k]->err; return rc; }
        }
        if (const int rc = place_search_reduce()) return rc;
        return copy_out();
    }
};

}  // namespace

extern "C" {

int emsar_hip_compare_groups_genes(emsar_hip_ctx *const *ctxs, int32_t n_samples, const int32_t *group_of, const double *size,
                                   const emsar_em_params *p, const emsar_groups_params *gp, int32_t n_query, const int32_t *query_genes,
                                   const emsar_groups_gene_outputs *out, emsar_groups_gene_stats *stats) {
    if (!ctxs || n_samples < 2 || n_samples > kGroupsMax || !group_of) return EMSAR_HIP_ERR_ARG;
    for (int k = 0; k < n_samples; k++) {
        if (!ctxs[k]) return EMSAR_HIP_ERR_ARG;
        for (int j = 0; j < k; j++) if (ctxs[j] == ctxs[k]) return EMSAR_HIP_ERR_ARG;
    }
    for (int k = 0; k < n_samples; k++) if (!ctxs[k]->have_sample) return EMSAR_HIP_ERR_STATE;
    for (int k = 1; k < n_samples; k++) if (ctxs[k]->device != ctxs[0]->device || !same_structure(ctxs[0], ctxs[k])) return EMSAR_HIP_ERR_ARG;
    const GeneMap &g0 = ctxs[0]->genes;
    if (!g0.have_genes) return EMSAR_HIP_ERR_STATE;
    for (int k = 1; k < n_samples; k++) {
        const GeneMap &gk = ctxs[k]->genes;
        if (gk.have_genes && (gk.n_genes != g0.n_genes || gk.h_gene_of_tx != g0.h_gene_of_tx)) return EMSAR_HIP_ERR_ARG;
    }
    if (const int rc = gene_query_ok(ctxs[0], n_query, query_genes)) return rc;
    const emsar_groups_params prm = groups_params_or_default(gp);
    if (!std::isfinite(prm.dev_tol)) return EMSAR_HIP_ERR_ARG;
    try {
        GroupsLayout L;
        if (!L.set(n_samples, group_of, size)) return EMSAR_HIP_ERR_ARG;
        for (int k = 1; k < n_samples; k++) if (const int rc = drain_stream(ctxs[k])) return rc;
        return run_query_call<GroupsGenesRun>(ctxs[0], stats, ctxs, L, p, prm, n_query, query_genes, out);
    } catch (const std::bad_alloc &) { return EMSAR_HIP_ERR_OOM; }
}

// Diagnostic only (not declared in the public header; makes no HIP call): what emsar_hip_compare_groups_genes gives a gene whose parts
// are all closed form in each of the K samples -- sample k has n_members[k] one-transcript components, (u, den) of all samples one
// sample behind the other -- the searches the host runs for such genes.  values[8]: lambda_between, p_between, lambda_within, p_within,
// raw_between, raw_within, gene_common, slope.  gene_group[G], gene_hat[K].  counts[4]: status, outer, evals, parts.
int emsar_hip_debug_compare_groups_genes_closed(int32_t n_samples, const int32_t *n_members, const double *u, const double *den,
                                                const int32_t *group_of, const double *size, const emsar_groups_params *gp, double *values,
                                                double *gene_group, double *gene_hat, int32_t *counts) {
    if (n_samples < 2 || n_samples > kGroupsMax || !n_members || !u || !den || !group_of || !values || !gene_group || !gene_hat || !counts)
        return EMSAR_HIP_ERR_ARG;
    const emsar_groups_params prm = groups_params_or_default(gp);
    if (!std::isfinite(prm.dev_tol)) return EMSAR_HIP_ERR_ARG;
    try {
        GroupsLayout L;
        if (!L.set(n_samples, group_of, size)) return EMSAR_HIP_ERR_ARG;
        std::vector<CompareGeneClosed> members[kGroupsMax];
        const CompareGeneClosed *cl[kGroupsMax];
        int n[kGroupsMax];
        double mn[kGroupsMax];
        size_t at = 0;
        int32_t parts = 0;
        for (int k = 0; k < n_samples; k++) {
            if (n_members[k] < 1 || n_members[k] > kGeneMaxParts) return EMSAR_HIP_ERR_ARG;
            mn[k] = INFINITY;
            for (int32_t i = 0; i < n_members[k]; i++, at++) {
                if (!(u[at] >= 0.0) || !(den[at] > 0.0)) return EMSAR_HIP_ERR_ARG;
                members[k].push_back(CompareGeneClosed{u[at], den[at]});
                mn[k] = std::min(mn[k], den[at]);
            }
            cl[k] = members[k].data(); n[k] = n_members[k]; parts += n_members[k];
        }
        GroupsResult o;
        if (!groups_closed_gene(L, cl, n, mn, groups_search_params(prm), o, gene_group, gene_hat)) return EMSAR_HIP_ERR_NUMERIC;
        const double v[8] = {o.lambda_between, groups_pvalue(o.lambda_between, L.G - 1), o.lambda_within, groups_pvalue(o.lambda_within, L.K - L.G),
                             o.raw_between, o.raw_within, o.theta_common, o.slope};
        for (int i = 0; i < 8; i++) values[i] = v[i];
        counts[0] = o.status; counts[1] = o.outer; counts[2] = o.evals; counts[3] = parts;
    } catch (const std::bad_alloc &) { return EMSAR_HIP_ERR_OOM; }
    return EMSAR_HIP_OK;
}

}  // extern "C"
