// fit.hpp -- the model fit behind include/emsar_hip.h: emsar_hip_model_fit (device) and emsar_hip_model_fit_host (no HIP call).  Part of
// emsar_hip.hip's translation unit, included at its end after resample.hpp: it uses the context, the gene map with launch_gene_sums, and
// the kernels of kernels_fit.hpp.
// One call = one FitRun:  check the arguments (host, before anything is uploaded)
//                         ensure_index   first call per structure: caller-order CSR and transposed index -> FitDev
//                         upload         theta, R, E of this call
//                         rows -> tx -> genes -> totals     (one HIP event between the stages)
//                         copy_out       library order -> caller order, statistics
// The context's own vectors are not touched: a following solve returns the same bits.

namespace {

bool fit_values_ok(const double *x, int64_t cnt) { return std::all_of(x, x + cnt, [](double v) { return std::isfinite(v) && v >= 0.0; }); }
bool fit_genes_all_or_none(const emsar_fit_outputs *o, bool &want) {
    const int given = o ? (o->gene_chi2 != nullptr) + (o->gene_dev != nullptr) + (o->gene_miss != nullptr) + (o->gene_df != nullptr) : 0;
    want = given == 4;
    return given == 0 || given == 4;
}
// rows that are not outside: not empty and E != 0
int64_t fit_rows_inside(int64_t n_rows, const uint64_t *row_ptr, const double *row_E) {
    int64_t n = 0;
    for (int64_t c = 0; c < n_rows; c++) n += row_ptr[c] < row_ptr[c + 1] && (!row_E || row_E[c] != 0.0);
    return n;
}

// the caller-order CSR of this structure on the device, once: the model fit and the asymptotic standard errors (asym.hpp) share it
int fit_ensure_csr(emsar_hip_ctx *ctx) {
    FitDev &F = ctx->fit;
    if (F.csr_ready) return EMSAR_HIP_OK;
    HIPCHK(F.d_row_ptr.upload(ctx->h_row_ptr.data(), (size_t)ctx->n_rows + 1));
    HIPCHK(F.d_col.upload(ctx->h_col.data(), (size_t)ctx->nnz));
    F.csr_ready = true;
    return EMSAR_HIP_OK;
}

struct FitRun {
    emsar_hip_ctx *const ctx;
    const double *const theta, *const row_E;
    const emsar_fit_outputs out;          // a copy: all NULL when the caller gave none
    const bool genes;
    const int64_t n_rows, n;              // rows, transcripts
    DevBuf<double> d_theta, d_E, d_rows, d_tx, d_gene, d_gpart, d_tot;   // [n] [n_rows] [3][n_rows] [4][n] [4][n_genes] [4][gene chunks] [4]
    DevBuf<int32_t> d_R, d_worst;                                        // [n_rows] [n]
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    emsar_fit_stats st{};

    FitRun(emsar_hip_ctx *c, const double *th, const double *E, const emsar_fit_outputs *o, bool want_genes)
        : ctx(c), theta(th), row_E(E), out(o ? *o : emsar_fit_outputs{}), genes(want_genes), n_rows(c->n_rows), n(c->n_tx) {}
    ~FitRun() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }

    // the caller-order CSR and the transposed index of this structure, once
    int ensure_index() {
        FitDev &F = ctx->fit;
        if (F.ready) return EMSAR_HIP_OK;
        if (const int rc = fit_ensure_csr(ctx)) return rc;
        emsar::FitIndex X;
        const int brc = emsar::build_fit_index(n_rows, ctx->n_tx, ctx->h_row_ptr.data(), ctx->h_col.data(), X);
        if (brc == -1) return EMSAR_HIP_ERR_OOM;
        if (brc != 0) { ctx->err = "model_fit: index builder: code " + std::to_string(brc); return EMSAR_HIP_ERR_HIP; }
        // results go to the library's index of a transcript: the [4][n_tx] block is what k_gene_sums reads
        const auto &m = tid_map(ctx);
        if (renumbered(ctx)) {
            for (auto &o : X.chunk_out) if (o >= 0) o = m[(size_t)o];
            for (size_t i = 0; i < X.multi.size(); i += 3) X.multi[i] = m[(size_t)X.multi[i]];
        }
        FitDev N;                    // the index: moved into the context, next to the CSR, when it is complete
        HIPCHK(N.d_idx.upload(X.idx.data(), X.idx.size()));
        HIPCHK(N.d_group_base.upload(X.group_base.data(), X.group_base.size()));
        HIPCHK(N.d_group_steps.upload(X.group_steps.data(), X.group_steps.size()));
        HIPCHK(N.d_chunk_tid.upload(X.chunk_tid.data(), X.chunk_tid.size()));
        HIPCHK(N.d_chunk_out.upload(X.chunk_out.data(), X.chunk_out.size()));
        HIPCHK(N.d_multi.upload(X.multi.data(), X.multi.size()));
        HIPCHK(N.d_rec.alloc((size_t)n_rows));
        if (X.n_multi > 0) { HIPCHK(N.d_part.alloc((size_t)(5 * X.n_chunks))); HIPCHK(N.d_part_row.alloc((size_t)X.n_chunks)); }
        N.n_chunks = X.n_chunks; N.n_groups = X.n_groups; N.n_multi = X.n_multi;
        N.index_slots = X.index_slots(); N.index_bytes = X.index_bytes();
        N.d_row_ptr = std::move(F.d_row_ptr); N.d_col = std::move(F.d_col);
        N.csr_ready = true; N.ready = true;
        ctx->fit = std::move(N);
        return EMSAR_HIP_OK;
    }

    int upload() {
        HIPCHK(d_theta.upload(theta, (size_t)n));
        HIPCHK(d_R.upload(ctx->h_wgt.data(), (size_t)n_rows));
        if (row_E) HIPCHK(d_E.upload(row_E, (size_t)n_rows));
        const int n_row_out = (out.row_mu != nullptr) + (out.row_chi2 != nullptr) + (out.row_dev != nullptr);
        if (n_row_out) HIPCHK(d_rows.alloc((size_t)(3 * n_rows)));
        HIPCHK(d_tx.alloc((size_t)(4 * n)));
        HIPCHK(d_worst.alloc((size_t)n));
        HIPCHK(d_tot.alloc(4));
        if (genes) {
            HIPCHK(d_gene.alloc((size_t)(4 * (int64_t)ctx->genes.n_genes)));
            if (ctx->genes.n_gene_multi > 0) HIPCHK(d_gpart.alloc((size_t)(4 * ctx->genes.n_gene_chunks)));
        }
        for (auto &e : ev) HIPCHK(hipEventCreate(&e));
        return EMSAR_HIP_OK;
    }

    int launch() {
        const FitDev &F = ctx->fit;
        hipStream_t s = ctx->stream;
        HIPCHK(hipEventRecord(ev[0], s));
        if (n_rows > 0)
            hipLaunchKernelGGL(k_fit_rows, dim3((unsigned)grid_for(n_rows, 256)), dim3(256), 0, s, n_rows, F.d_row_ptr.get(), F.d_col.get(), d_R.get(),
                               row_E ? d_E.get() : nullptr, d_theta.get(), F.d_rec.get(), out.row_mu ? d_rows.get() : nullptr,
                               out.row_chi2 ? d_rows + n_rows : nullptr, out.row_dev ? d_rows + 2 * n_rows : nullptr);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev[1], s));
        if (F.n_chunks > 0)
            hipLaunchKernelGGL(k_fit_tx, dim3((unsigned)grid_for(F.n_chunks, 256)), dim3(256), 0, s, F.n_chunks, F.d_idx.get(), F.d_group_base.get(),
                               F.d_group_steps.get(), F.d_chunk_tid.get(), F.d_chunk_out.get(), d_theta.get(), F.d_rec.get(), n, d_tx.get(),
                               d_worst.get(), F.d_part.get(), F.d_part_row.get());
        if (F.n_multi > 0)
            hipLaunchKernelGGL(k_fit_tx_finish, dim3((unsigned)grid_for(F.n_multi, 256)), dim3(256), 0, s, F.n_multi, F.d_multi.get(), F.d_part.get(),
                               F.d_part_row.get(), F.n_chunks, n, d_tx.get(), d_worst.get());
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev[2], s));
        if (genes) { const int rc = launch_gene_sums(ctx, d_tx, 4, d_gene, d_gpart); if (rc) return rc; }
        HIPCHK(hipEventRecord(ev[3], s));
        hipLaunchKernelGGL(k_fit_totals, dim3(1), dim3(1024), 0, s, n_rows, F.d_rec.get(), d_tot.get());
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev[4], s));
        return EMSAR_HIP_OK;
    }

    int copy_out() {
        const FitDev &F = ctx->fit;
        hipStream_t s = ctx->stream;
        const int64_t ng = genes ? ctx->genes.n_genes : 0;
        std::vector<double> tx((size_t)(4 * n)), gene((size_t)(4 * ng));
        std::vector<int32_t> worst((size_t)n);
        double tot[4] = {0.0, 0.0, 0.0, 0.0};
        double *const rows[3] = {out.row_mu, out.row_chi2, out.row_dev};
        for (int k = 0; k < 3; k++)
            if (rows[k] && n_rows > 0) HIPCHK(hipMemcpyAsync(rows[k], d_rows + k * n_rows, (size_t)n_rows * 8, hipMemcpyDeviceToHost, s));
        if (n > 0) {
            HIPCHK(hipMemcpyAsync(tx.data(), d_tx, tx.size() * 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(worst.data(), d_worst, worst.size() * 4, hipMemcpyDeviceToHost, s));
        }
        if (ng > 0) HIPCHK(hipMemcpyAsync(gene.data(), d_gene, gene.size() * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(tot, d_tot, sizeof tot, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        // library order -> caller order
        const auto &m = tid_map(ctx);
        const bool remap = renumbered(ctx);
        double *const txo[4] = {out.tx_chi2, out.tx_dev, out.tx_miss, out.tx_df};
        for (int64_t t = 0; t < n; t++) {
            const size_t l = remap ? (size_t)m[(size_t)t] : (size_t)t;
            for (int k = 0; k < 4; k++) if (txo[k]) txo[k][t] = tx[(size_t)(k * n) + l];
            if (out.tx_worst_row) out.tx_worst_row[t] = worst[l];
        }
        if (genes) {
            double *const go[4] = {out.gene_chi2, out.gene_dev, out.gene_miss, out.gene_df};
            for (int k = 0; k < 4; k++) std::copy(gene.begin() + k * ng, gene.begin() + (k + 1) * ng, go[k]);
        }
        float ms[4] = {0, 0, 0, 0}, all = 0;
        for (int k = 0; k < 4; k++) HIPCHK(hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]));
        HIPCHK(hipEventElapsedTime(&all, ev[0], ev[4]));
        st.kernel_ms = all; st.rows_ms = ms[0]; st.tx_ms = ms[1]; st.genes_ms = ms[2]; st.totals_ms = ms[3];
        st.sum_chi2 = tot[0]; st.sum_dev = tot[1]; st.sum_miss = tot[2]; st.rows_infeasible = (int64_t)tot[3];
        st.index_slots = F.index_slots; st.index_bytes = F.index_bytes;
        return EMSAR_HIP_OK;
    }
};

}  // namespace

extern "C" {

int emsar_hip_model_fit(emsar_hip_ctx *ctx, const double *theta, const double *row_E, const emsar_fit_outputs *out, emsar_fit_stats *stats) {
    if (!ctx) return EMSAR_HIP_ERR_ARG;
    if (!ctx->have_sample) return EMSAR_HIP_ERR_STATE;
    bool want_genes = false;
    if (!theta || ctx->n_rows > (int64_t)INT32_MAX || !fit_genes_all_or_none(out, want_genes)) return EMSAR_HIP_ERR_ARG;
    if (!fit_values_ok(theta, ctx->n_tx) || (row_E && !fit_values_ok(row_E, ctx->n_rows))) return EMSAR_HIP_ERR_ARG;
    if (want_genes && !ctx->genes.have_genes) return EMSAR_HIP_ERR_STATE;
    const auto t0 = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    try {
        FitRun run(ctx, theta, row_E, out, want_genes);
        int rc;
        if ((rc = run.ensure_index()) || (rc = run.upload()) || (rc = run.launch()) || (rc = run.copy_out())) return rc;
        run.st.rows_inside = fit_rows_inside(ctx->n_rows, ctx->h_row_ptr.data(), row_E);
        run.st.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = run.st;
    } catch (const std::bad_alloc &) { return EMSAR_HIP_ERR_OOM; }
    return EMSAR_HIP_OK;
}

// The same definition on the host: fit_index.hpp's functions in loops over the rows, the chunks in the index' order, the transcripts
// of more than one chunk, and the genes' chunked sums.
int emsar_hip_model_fit_host(int64_t n_rows, int32_t n_tx, const uint64_t *row_ptr, const int32_t *col_idx, const int32_t *row_weight,
                             const double *row_E, const double *theta, int32_t n_genes, const int32_t *gene_of_tx,
                             const emsar_fit_outputs *out, emsar_fit_stats *stats) {
    bool want_genes = false;
    if (!theta || n_rows > (int64_t)INT32_MAX || !fit_genes_all_or_none(out, want_genes)) return EMSAR_HIP_ERR_ARG;
    if (emsar::validate_csr(n_rows, n_tx, row_ptr, col_idx) != 0) return EMSAR_HIP_ERR_ARG;
    if (!fit_values_ok(theta, n_tx) || (row_E && !fit_values_ok(row_E, n_rows))) return EMSAR_HIP_ERR_ARG;
    if (row_weight) for (int64_t c = 0; c < n_rows; c++) if (row_weight[c] < 0) return EMSAR_HIP_ERR_ARG;
    if (gene_of_tx) {
        if (n_genes < 1) return EMSAR_HIP_ERR_ARG;
        for (int32_t t = 0; t < n_tx; t++) if (gene_of_tx[t] < -1 || gene_of_tx[t] >= n_genes) return EMSAR_HIP_ERR_ARG;
    } else if (want_genes) return EMSAR_HIP_ERR_STATE;
    const auto t0 = std::chrono::steady_clock::now();
    const emsar_fit_outputs o = out ? *out : emsar_fit_outputs{};
    try {
        emsar::FitIndex X;
        const int brc = emsar::build_fit_index(n_rows, n_tx, row_ptr, col_idx, X);
        if (brc == -1) return EMSAR_HIP_ERR_OOM;
        if (brc != 0) return EMSAR_HIP_ERR_HIP;
        // stage 1: the rows
        std::vector<emsar::FitRec> rec((size_t)n_rows);
        for (int64_t c = 0; c < n_rows; c++) {
            const double E = row_E ? row_E[c] : 1.0;
            emsar::FitRec x = {0.0, 0.0, 0.0, 0.0};
            double mu = 0.0;
            if (row_ptr[c] < row_ptr[c + 1] && E != 0.0) {
                double S = 0.0;
                for (uint64_t k = row_ptr[c]; k < row_ptr[c + 1]; k++) S = S + theta[col_idx[k]];
                x.S = emsar::fit_row_terms((double)(row_weight ? row_weight[c] : 1), E, S, &mu, &x.q, &x.d, &x.a);
            }
            rec[(size_t)c] = x;
            if (o.row_mu) o.row_mu[c] = mu;
            if (o.row_chi2) o.row_chi2[c] = x.q;
            if (o.row_dev) o.row_dev[c] = x.d;
        }
        // stage 2: the chunks, then the transcripts of more than one
        const int64_t nc = X.n_chunks, T = n_tx;
        std::vector<double> tx((size_t)(4 * T)), part((size_t)(X.n_multi > 0 ? 5 * nc : 0));
        std::vector<int32_t> worst((size_t)T), part_row((size_t)(X.n_multi > 0 ? nc : 0));
        auto put = [&](int32_t t, const emsar::FitAcc &A) {
            tx[(size_t)t] = A.chi2; tx[(size_t)(T + t)] = A.dev; tx[(size_t)(2 * T + t)] = A.miss; tx[(size_t)(3 * T + t)] = A.df;
            worst[(size_t)t] = A.row;
        };
        for (int64_t s = 0; s < nc; s++) {
            const int64_t g = s / emsar::kFitGroup;
            const emsar::FitAcc A = emsar::fit_walk_chunk(X.idx.data(), X.group_base[(size_t)g] + s % emsar::kFitGroup, X.group_steps[(size_t)g],
                                                          theta[X.chunk_tid[(size_t)s]], rec.data());
            const int32_t co = X.chunk_out[(size_t)s];
            if (co >= 0) put(co, A);
            else {
                const int64_t k = -1 - (int64_t)co;
                part[(size_t)k] = A.chi2; part[(size_t)(nc + k)] = A.dev; part[(size_t)(2 * nc + k)] = A.miss; part[(size_t)(3 * nc + k)] = A.df;
                part[(size_t)(4 * nc + k)] = A.best;
                part_row[(size_t)k] = A.row;
            }
        }
        for (int64_t i = 0; i < X.n_multi; i++)
            put(X.multi[(size_t)(3 * i)], emsar::fit_finish(part.data(), part_row.data(), nc, X.multi[(size_t)(3 * i + 1)], X.multi[(size_t)(3 * i + 2)]));
        double *const txo[4] = {o.tx_chi2, o.tx_dev, o.tx_miss, o.tx_df};
        for (int k = 0; k < 4; k++) if (txo[k]) std::copy(tx.begin() + k * T, tx.begin() + (k + 1) * T, txo[k]);
        if (o.tx_worst_row) std::copy(worst.begin(), worst.end(), o.tx_worst_row);
        // the genes: gene_sums' order -- ascending tid, chunks of kGeneChunk left to right, then the chunk sums left to right
        if (want_genes) {
            std::vector<int64_t> gp((size_t)n_genes + 1, 0);
            for (int32_t t = 0; t < n_tx; t++) if (gene_of_tx[t] >= 0) gp[(size_t)gene_of_tx[t] + 1]++;
            for (int32_t g = 0; g < n_genes; g++) gp[(size_t)g + 1] += gp[(size_t)g];
            std::vector<int32_t> gtx((size_t)gp[(size_t)n_genes]);
            std::vector<int64_t> fill(gp.begin(), gp.end() - 1);
            for (int32_t t = 0; t < n_tx; t++) if (gene_of_tx[t] >= 0) gtx[(size_t)fill[(size_t)gene_of_tx[t]]++] = t;
            double *const go[4] = {o.gene_chi2, o.gene_dev, o.gene_miss, o.gene_df};
            for (int k = 0; k < 4; k++) {
                const double *x = tx.data() + k * T;
                for (int32_t g = 0; g < n_genes; g++) {
                    double sum = 0.0;
                    for (int64_t b = gp[(size_t)g]; b < gp[(size_t)g + 1]; b += kGeneChunk) {
                        const int64_t e = std::min<int64_t>(b + kGeneChunk, gp[(size_t)g + 1]);
                        double s = x[gtx[(size_t)b]];
                        for (int64_t i = b + 1; i < e; i++) s += x[gtx[(size_t)i]];
                        sum = b == gp[(size_t)g] ? s : sum + s;
                    }
                    go[k][g] = sum;
                }
            }
        }
        if (stats) {
            double tot[4];
            emsar::fit_totals_host(rec.data(), n_rows, tot);
            emsar_fit_stats st{};
            st.rows_inside = fit_rows_inside(n_rows, row_ptr, row_E);
            st.rows_infeasible = (int64_t)tot[3];
            st.sum_chi2 = tot[0]; st.sum_dev = tot[1]; st.sum_miss = tot[2];
            st.index_slots = X.index_slots(); st.index_bytes = X.index_bytes();
            st.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            *stats = st;
        }
    } catch (const std::bad_alloc &) { return EMSAR_HIP_ERR_OOM; }
    return EMSAR_HIP_OK;
}

}  // extern "C"
