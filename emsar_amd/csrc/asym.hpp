// asym.hpp -- the asymptotic standard errors behind include/emsar_hip.h: emsar_hip_asymptotic (device) and emsar_hip_asymptotic_host
// (no HIP call).  Part of emsar_hip.hip's translation unit, included at its end after presence.hpp: it uses the context, the shared
// caller-order CSR (fit.hpp: fit_ensure_csr), the gene map with launch_gene_sums, and the kernels of kernels_asym.hpp.
// One call = one AsymRun:  plan      (host) active set, components, packed records; every index checked before anything is launched
//                          upload    theta, R, the records, the items of every kernel class
//                          rows -> sets -> genes     (one HIP event between the stages; the classes next to each other on their streams)
//                          finish    (host) slots -> caller order, asym_finish, copy_out, statistics
// The context's own vectors are not touched: a following solve returns the same bits.

namespace {

bool asym_groups_ok(const emsar_asym_outputs *o, bool &want_genes, bool &want_block) {
    const int g = o ? (o->gene_sd != nullptr) + (o->gene_status != nullptr) : 0;
    const int b = o ? (o->block_n != nullptr) + (o->block_tids != nullptr) + (o->block_cov != nullptr) : 0;
    want_genes = g == 2 || (o && o->usage_sd);
    want_block = b == 3;
    return (g == 0 || g == 2) && (b == 0 || b == 3);
}
emsar_asym_params asym_defaults(const emsar_asym_params *p) {
    emsar_asym_params q = p ? *p : emsar_asym_params{EMSAR_ASYM_DEFAULT_CUT, 0.0, -1, 0};
    if (!(q.pivot_tol > 0.0)) q.pivot_tol = 1e-10;
    return q;
}

// What both paths do once the slots and the descriptors' flags are known: caller order, the finish, the outputs, the statistics.
// VG [n_genes] or null: the gene sums of genesum when the device made them, else they are made here.  block [n * n] of block_desc.
void asym_deliver(const emsar::AsymPlan &P, int32_t n_tx, const double *theta, const emsar_asym_params &q, const double *s_var,
                  const double *s_rowsum, const double *s_gsum, const double *s_pcov, const int32_t *s_partner, const int32_t *c_fail,
                  const double *c_ratio, int32_t n_genes, const int32_t *gene_of_tx, const double *VG, const double *block,
                  const emsar_asym_outputs &o, emsar_asym_stats &st) {
    emsar::AsymTx R;
    emsar::asym_assemble(P, n_tx, s_var, s_rowsum, s_gsum, s_pcov, s_partner, c_fail, R);
    emsar::AsymGenes genes;
    std::vector<double> vg;
    if (gene_of_tx) {
        genes.build(n_tx, n_genes, gene_of_tx);
        if (!VG) {
            vg.resize((size_t)n_genes);
            for (int32_t g = 0; g < n_genes; g++) vg[(size_t)g] = genes.sum(g, R.genesum.data());
            VG = vg.data();
        }
    }
    emsar::asym_finish(n_tx, theta, R, n_genes, gene_of_tx, &genes, VG, o.sd_fpkm, o.sd_tpm, gene_of_tx ? o.usage_sd : nullptr, o.gene_sd,
                       o.gene_status, &st.theta_unestimated_share);
    const size_t T = (size_t)n_tx;
    if (o.var) std::copy(R.var.begin(), R.var.end(), o.var);
    if (o.rowsum) std::copy(R.rowsum.begin(), R.rowsum.end(), o.rowsum);
    if (o.status) std::copy(R.status.begin(), R.status.end(), o.status);
    if (o.partner) std::copy(R.partner.begin(), R.partner.end(), o.partner);
    if (o.partner_cov) std::copy(R.pcov.begin(), R.pcov.end(), o.partner_cov);
    if (o.blocker) std::copy(R.blocker.begin(), R.blocker.end(), o.blocker);
    if (o.block_n) {
        *o.block_n = 0;
        const int32_t c = q.block_tid >= 0 ? P.comp_of[(size_t)q.block_tid] : -1;
        if (c >= 0 && c_fail[c] < 0) {
            const emsar::AsymDesc &d = P.desc[(size_t)c];
            *o.block_n = (int32_t)d.n;
            std::copy(P.g_tid.begin() + d.tid_off, P.g_tid.begin() + d.tid_off + d.n, o.block_tids);
            std::copy(block, block + (size_t)d.n * d.n, o.block_cov);
        }
    }
    st.components = P.components; st.components_too_large = P.too_large; st.components_infeasible = P.infeasible;
    st.rows_infeasible = P.rows_infeasible; st.max_n = P.max_n;
    st.min_pivot_ratio = INFINITY;
    for (size_t c = 0; c < P.desc.size(); c++) {
        st.components_unidentifiable += c_fail[c] >= 0;
        if (c_ratio[c] < st.min_pivot_ratio) st.min_pivot_ratio = c_ratio[c];
    }
    for (size_t t = 0; t < T; t++) st.n_status[R.status[t]]++;
}

struct AsymRun {
    emsar_hip_ctx *const ctx;
    const double *const theta;
    const emsar_asym_params q;            // the caller's parameters with the defaults filled in
    const emsar_asym_outputs out;         // a copy: all NULL when the caller gave none
    const bool genes, want_block;
    const int64_t n_rows;
    const int32_t n;
    emsar::AsymPlan P;
    std::vector<uint32_t> items[emsar::kAsymClasses];
    std::vector<int32_t> h_lib, h_gene;   // [slots]
    int32_t block_desc = -1;
    size_t lds[emsar::kAsymClasses] = {0, 0, 0, 0};
    DevBuf<double> d_theta, d_w, d_slot, d_ratio, d_gsum_lib, d_vg, d_gpart, d_block;     // d_slot [4][slots]: var, rowsum, gsum, pcov
    DevBuf<int32_t> d_R, d_crow, d_gene, d_lib, d_partner, d_fail;
    DevBuf<uint32_t> d_rp, d_tp, d_tent, d_items[emsar::kAsymClasses];
    DevBuf<uint8_t> d_ids;
    DevBuf<emsar::AsymDesc> d_desc;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    emsar_asym_stats st{};

    AsymRun(emsar_hip_ctx *c, const double *th, const emsar_asym_params *p, const emsar_asym_outputs *o, bool want_genes, bool want_blk)
        : ctx(c), theta(th), q(asym_defaults(p)), out(o ? *o : emsar_asym_outputs{}), genes(want_genes), want_block(want_blk),
          n_rows(c->n_rows), n(c->n_tx) {}
    ~AsymRun() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }

    int plan() {
        const auto t0 = std::chrono::steady_clock::now();
        const int brc = emsar::asym_build_plan(n_rows, n, ctx->h_row_ptr.data(), ctx->h_col.data(), ctx->h_wgt.data(), theta, q.boundary_cut, P);
        if (brc != 0) { ctx->err = "asymptotic: the components' records do not fit 32-bit offsets"; return EMSAR_HIP_ERR_OOM; }
        if (const int crc = emsar::asym_check_plan(P, n_rows, n)) { ctx->err = "asymptotic: record check: code " + std::to_string(crc); return EMSAR_HIP_ERR_HIP; }
        // EMSAR_HIP_ASYM_CLASS = 1 | 2: every component in at least the one-wave / the 256-thread kernel
        int floor_cls = 0;
        if (const char *env = getenv("EMSAR_HIP_ASYM_CLASS")) { const int v = atoi(env); if (v == 1 || v == 2) floor_cls = v + 1; }
        for (size_t c = 0; c < P.desc.size(); c++) {
            const int nn = (int)P.desc[c].n, cls = std::max(emsar::asym_class_of(nn), floor_cls);
            items[cls].push_back((uint32_t)c);
            st.components_class[cls]++;
            if (cls >= 2) lds[cls] = std::max(lds[cls], (size_t)(nn * (nn + 1) / 2 + 2 * nn) * 8);
        }
        lds[1] = (size_t)8 * (36 + 16) * 8;
        const auto &m = tid_map(ctx);
        const bool remap = renumbered(ctx);
        h_lib.resize(P.slots()); h_gene.resize(P.slots());
        for (size_t s = 0; s < P.slots(); s++) {
            const int32_t t = P.g_tid[s];
            h_lib[s] = remap ? m[(size_t)t] : t;
            h_gene[s] = genes ? ctx->genes.h_gene_of_tx[(size_t)t] : -1;
        }
        if (want_block && q.block_tid >= 0) block_desc = P.comp_of[(size_t)q.block_tid];
        st.plan_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return EMSAR_HIP_OK;
    }

    int upload() {
        int rc;
        if ((rc = fit_ensure_csr(ctx))) return rc;
        const size_t slots = P.slots(), nd = P.desc.size();
        HIPCHK(d_theta.upload(theta, (size_t)n));
        HIPCHK(d_R.upload(ctx->h_wgt.data(), (size_t)n_rows));
        HIPCHK(d_w.alloc((size_t)n_rows));
        HIPCHK(d_desc.upload(P.desc.data(), nd));
        HIPCHK(d_crow.upload(P.crow.data(), P.crow.size()));
        HIPCHK(d_rp.upload(P.rp.data(), P.rp.size()));
        HIPCHK(d_tp.upload(P.tp.data(), P.tp.size()));
        HIPCHK(d_tent.upload(P.tent.data(), P.tent.size()));
        HIPCHK(d_ids.upload(P.ids.data(), P.ids.size()));
        HIPCHK(d_gene.upload(h_gene.data(), slots));
        HIPCHK(d_lib.upload(h_lib.data(), slots));
        for (int c = 0; c < emsar::kAsymClasses; c++) if (!items[c].empty()) HIPCHK(d_items[c].upload(items[c].data(), items[c].size()));
        HIPCHK(d_slot.alloc(4 * slots)); HIPCHK(d_partner.alloc(slots));
        HIPCHK(d_fail.alloc(nd)); HIPCHK(d_ratio.alloc(nd));
        HIPCHK(d_block.alloc((size_t)emsar::kAsymMaxN * emsar::kAsymMaxN));
        if (genes) {
            HIPCHK(d_gsum_lib.alloc((size_t)n));
            HIPCHK(hipMemsetAsync(d_gsum_lib, 0, (size_t)std::max(n, 2) * 8, ctx->stream));
            HIPCHK(d_vg.alloc((size_t)ctx->genes.n_genes));
            if (ctx->genes.n_gene_multi > 0) HIPCHK(d_gpart.alloc((size_t)ctx->genes.n_gene_chunks));
        }
        for (auto &e : ev) HIPCHK(hipEventCreate(&e));
        return EMSAR_HIP_OK;
    }

    int launch() {
        const FitDev &F = ctx->fit;
        hipStream_t s = ctx->stream;
        const size_t slots = P.slots();
        HIPCHK(hipFuncSetAttribute((const void *)k_asym_sets<256, 256>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)((emsar::kAsymMaxN * (emsar::kAsymMaxN + 1) / 2 + 2 * emsar::kAsymMaxN) * 8)));
        HIPCHK(hipEventRecord(ev[0], s));
        if (n_rows > 0)
            hipLaunchKernelGGL(k_asym_rows, dim3((unsigned)grid_for(n_rows, 256)), dim3(256), 0, s, n_rows, F.d_row_ptr.get(), F.d_col.get(), d_R.get(),
                               d_theta.get(), d_w.get());
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev[1], s));
        const emsar::AsymRecords X{d_desc.get(), d_crow.get(), genes ? d_gene.get() : nullptr, d_rp.get(), d_tp.get(), d_tent.get(), d_ids.get()};
        const AsymOut O{d_slot.get(), d_slot + slots, d_slot + 2 * slots, d_slot + 3 * slots, d_partner.get(), d_fail.get(), d_ratio.get(), d_lib.get(),
                        genes ? d_gsum_lib.get() : nullptr, d_block.get(), block_desc};
        // the classes are independent (disjoint components, disjoint slots): the two larger ones run on side streams
        int rc;
        if ((rc = fork_side_streams(ctx, 2))) return rc;
        const int64_t cnt[emsar::kAsymClasses] = {(int64_t)items[0].size(), (int64_t)items[1].size(), (int64_t)items[2].size(), (int64_t)items[3].size()};
        if (cnt[3]) hipLaunchKernelGGL((k_asym_sets<256, 256>), dim3((unsigned)cnt[3]), dim3(256), lds[3], ctx->side[1], X, d_items[3].get(), cnt[3], d_w.get(), q.pivot_tol, O);
        if (cnt[2]) hipLaunchKernelGGL((k_asym_sets<64, 64>), dim3((unsigned)cnt[2]), dim3(64), lds[2], ctx->side[0], X, d_items[2].get(), cnt[2], d_w.get(), q.pivot_tol, O);
        if (cnt[1]) hipLaunchKernelGGL((k_asym_sets<8, 64>), dim3((unsigned)grid_for(cnt[1], 8)), dim3(64), lds[1], s, X, d_items[1].get(), cnt[1], d_w.get(), q.pivot_tol, O);
        if (cnt[0]) hipLaunchKernelGGL(k_asym_single, dim3((unsigned)grid_for(cnt[0], 256)), dim3(256), 0, s, X, d_items[0].get(), cnt[0], d_w.get(), q.pivot_tol, O);
        HIPCHK(hipGetLastError());
        for (int i = 0; i < 2; i++) {
            HIPCHK(hipEventRecord(ctx->ev_join[i], ctx->side[i]));
            HIPCHK(hipStreamWaitEvent(s, ctx->ev_join[i], 0));
        }
        HIPCHK(hipEventRecord(ev[2], s));
        if (genes && (rc = launch_gene_sums(ctx, d_gsum_lib, 1, d_vg, d_gpart))) return rc;
        HIPCHK(hipEventRecord(ev[3], s));
        return EMSAR_HIP_OK;
    }

    int finish() {
        hipStream_t s = ctx->stream;
        const size_t slots = P.slots(), nd = P.desc.size();
        const int32_t ng = genes ? ctx->genes.n_genes : 0;
        // a slot of a component that failed its pivot test is never written, and never read
        std::vector<double> slot(4 * slots, 0.0), ratio(nd), vg((size_t)ng), block;
        std::vector<int32_t> partner(slots, -1), fail(nd);
        if (slots > 0) {
            HIPCHK(hipMemcpyAsync(slot.data(), d_slot, slot.size() * 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(partner.data(), d_partner, slots * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(fail.data(), d_fail, nd * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(ratio.data(), d_ratio, nd * 8, hipMemcpyDeviceToHost, s));
        }
        if (ng > 0) HIPCHK(hipMemcpyAsync(vg.data(), d_vg, (size_t)ng * 8, hipMemcpyDeviceToHost, s));
        if (block_desc >= 0) {
            const size_t bn = P.desc[(size_t)block_desc].n;
            block.resize(bn * bn);
            HIPCHK(hipMemcpyAsync(block.data(), d_block, bn * bn * 8, hipMemcpyDeviceToHost, s));
        }
        HIPCHK(hipStreamSynchronize(s));
        asym_deliver(P, n, theta, q, slot.data(), slot.data() + slots, slot.data() + 2 * slots, slot.data() + 3 * slots, partner.data(), fail.data(),
                     ratio.data(), ng, genes ? ctx->genes.h_gene_of_tx.data() : nullptr, genes ? vg.data() : nullptr, block.data(), out, st);
        float ms[3] = {0, 0, 0};
        for (int k = 0; k < 3; k++) HIPCHK(hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]));
        st.rows_ms = ms[0]; st.sets_ms = ms[1]; st.genes_ms = ms[2];
        return EMSAR_HIP_OK;
    }
};

bool asym_theta_ok(const double *theta, const emsar_asym_params *p, int32_t n_tx) {
    if (!theta || !fit_values_ok(theta, n_tx)) return false;
    if (p && (p->block_tid < -1 || p->block_tid >= n_tx || p->boundary_cut != p->boundary_cut || p->pivot_tol != p->pivot_tol)) return false;
    return true;
}

}  // namespace

extern "C" {

int emsar_hip_asymptotic(emsar_hip_ctx *ctx, const double *theta, const emsar_asym_params *params, const emsar_asym_outputs *out,
                         emsar_asym_stats *stats) {
    if (!ctx) return EMSAR_HIP_ERR_ARG;
    if (!ctx->have_sample) return EMSAR_HIP_ERR_STATE;
    bool want_genes = false, want_block = false;
    if (!asym_groups_ok(out, want_genes, want_block) || !asym_theta_ok(theta, params, ctx->n_tx)) return EMSAR_HIP_ERR_ARG;
    if (want_genes && !ctx->genes.have_genes) return EMSAR_HIP_ERR_STATE;
    const auto t0 = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    try {
        // with a gene map the gene sums are always formed: genesum is part of no output, but usage_sd and gene_sd hang on it
        AsymRun run(ctx, theta, params, out, ctx->genes.have_genes, want_block);
        int rc;
        if ((rc = run.plan()) || (rc = run.upload()) || (rc = run.launch()) || (rc = run.finish())) return rc;
        run.st.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = run.st;
    } catch (const std::bad_alloc &) { return EMSAR_HIP_ERR_OOM; }
    return EMSAR_HIP_OK;
}

// The same definition on the host: asym_plan.hpp's functions in loops over the rows and the components.
int emsar_hip_asymptotic_host(int64_t n_rows, int32_t n_tx, const uint64_t *row_ptr, const int32_t *col_idx, const int32_t *row_weight,
                              const double *row_E, const double *theta, int32_t n_genes, const int32_t *gene_of_tx,
                              const emsar_asym_params *params, const emsar_asym_outputs *out, emsar_asym_stats *stats) {
    bool want_genes = false, want_block = false;
    if (!asym_groups_ok(out, want_genes, want_block)) return EMSAR_HIP_ERR_ARG;
    if (emsar::validate_csr(n_rows, n_tx, row_ptr, col_idx) != 0) return EMSAR_HIP_ERR_ARG;
    if (!asym_theta_ok(theta, params, n_tx)) return EMSAR_HIP_ERR_ARG;
    if (row_weight) for (int64_t c = 0; c < n_rows; c++) if (row_weight[c] < 0) return EMSAR_HIP_ERR_ARG;
    if (gene_of_tx) {
        if (n_genes < 1) return EMSAR_HIP_ERR_ARG;
        for (int32_t t = 0; t < n_tx; t++) if (gene_of_tx[t] < -1 || gene_of_tx[t] >= n_genes) return EMSAR_HIP_ERR_ARG;
    } else if (want_genes) return EMSAR_HIP_ERR_STATE;
    const auto t0 = std::chrono::steady_clock::now();
    const emsar_asym_outputs o = out ? *out : emsar_asym_outputs{};
    const emsar_asym_params q = asym_defaults(params);
    try {
        emsar_asym_stats st{};
        std::vector<int32_t> wgt((size_t)n_rows);
        for (int64_t c = 0; c < n_rows; c++) wgt[(size_t)c] = (row_E && row_E[c] == 0.0) ? 0 : row_weight ? row_weight[c] : 1;
        emsar::AsymPlan P;
        if (emsar::asym_build_plan(n_rows, n_tx, row_ptr, col_idx, wgt.data(), theta, q.boundary_cut, P) != 0) return EMSAR_HIP_ERR_OOM;
        if (emsar::asym_check_plan(P, n_rows, n_tx) != 0) return EMSAR_HIP_ERR_HIP;
        st.plan_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        std::vector<double> w((size_t)n_rows);
        for (int64_t c = 0; c < n_rows; c++) {
            double S = 0.0;
            for (uint64_t k = row_ptr[c]; k < row_ptr[c + 1]; k++) S = S + theta[col_idx[k]];
            w[(size_t)c] = emsar::asym_row_w((double)wgt[(size_t)c], S);
        }
        const size_t slots = P.slots(), nd = P.desc.size();
        std::vector<int32_t> gene(slots, -1), partner(slots, -1), fail(nd);
        if (gene_of_tx) for (size_t s = 0; s < slots; s++) gene[s] = gene_of_tx[P.g_tid[s]];
        std::vector<double> slot(4 * slots, 0.0), ratio(nd), A, D, diag, block;
        const emsar::AsymRecords X{P.desc.data(), P.crow.data(), gene_of_tx ? gene.data() : nullptr, P.rp.data(), P.tp.data(), P.tent.data(), P.ids.data()};
        const int32_t block_desc = (want_block && q.block_tid >= 0) ? P.comp_of[(size_t)q.block_tid] : -1;
        for (size_t c = 0; c < nd; c++) {
            fail[c] = emsar::asym_eval_component(X, P.desc[c], w.data(), q.pivot_tol, A, D, diag, slot.data(), slot.data() + slots,
                                                 slot.data() + 2 * slots, slot.data() + 3 * slots, partner.data(), &ratio[c]);
            st.components_class[emsar::asym_class_of((int)P.desc[c].n)]++;
            if ((int32_t)c == block_desc && fail[c] < 0) {
                const int bn = (int)P.desc[c].n;
                block.resize((size_t)bn * bn);
                for (int i = 0; i < bn; i++) for (int j = 0; j < bn; j++) block[(size_t)(i * bn + j)] = A[(size_t)(i >= j ? emsar::asym_tri(i, j) : emsar::asym_tri(j, i))];
            }
        }
        asym_deliver(P, n_tx, theta, q, slot.data(), slot.data() + slots, slot.data() + 2 * slots, slot.data() + 3 * slots, partner.data(), fail.data(),
                     ratio.data(), n_genes, gene_of_tx, nullptr, block.data(), o, st);
        st.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = st;
    } catch (const std::bad_alloc &) { return EMSAR_HIP_ERR_OOM; }
    return EMSAR_HIP_OK;
}

}  // extern "C"
