// resample.hpp -- the resampling driver behind include/emsar_hip.h: the Poisson bootstrap, its gene-level statistics and quantiles, the
// binomial depth subsampling, and the gene map with its sums.  Part of emsar_hip.hip's translation unit, included at its end: it uses
// the context, layout_weights, plan_solve and SolveRun (solve.hpp) and the kernels (kernels_boot.hpp, kernels_genes.hpp, kernels_quant.hpp,
// kernels_isoforms.hpp).
// One call = one BootRun:  plan memory (held replicates first, then the batch size) -> allocate
//                          for each fraction:  zero the accumulators
//                              for each batch:  draw -> solve_sets -> solve_streamed -> reduce -> copy_out
//                              finish_round (means / sd, gene outputs, depth_mean);  quantiles (if the replicates are held)
//                          fill the statistics; put the context back (BootRestore)
// The isoform usage (emsar_hip_isoform_usage, emsar_hip_bootstrap_isoforms) rides on the same stages: reduce and quantiles.

namespace {

// The sample's row weights in caller order on the device (the draws' R) and, for the set solver, the draw map: build_sets run again
// on the same weights with the map asked for -- the same code that filled row_w / usum, so the same sets, merged rows and slots.
int boot_prepare(emsar_hip_ctx *ctx, bool want_slot) {
    if (!ctx->sets.d_boot_R) HIPCHK(ctx->sets.d_boot_R.upload(ctx->h_wgt.data(), (size_t)ctx->n_rows));
    if (!want_slot || ctx->sets.boot_slot_ready) return EMSAR_HIP_OK;
    try {
        emsar::ResidentSets S;
        std::vector<int64_t> slot;
        emsar::build_sets(ctx->n_rows, ctx->n_tx, ctx->h_row_ptr.data(), ctx->h_col.data(), ctx->h_wgt.data(), S, &slot);
        const int64_t n_rw = (int64_t)S.row_w.size();
        // the resident records on the device are those of ensure_sets: same input, same builder
        size_t rw_dev = 0;
        for (int c = 0; c < emsar::kSetClasses; c++) for (const auto &d : S.desc[c]) rw_dev += d.n_r;
        if (rw_dev != (size_t)n_rw || S.n_resident() != ctx->sets.RS.n_resident()) { ctx->err = "bootstrap: draw map does not match the sets"; return EMSAR_HIP_ERR_HIP; }
        const auto &m = tid_map(ctx);
        const bool remap = renumbered(ctx);
        for (auto &v : slot)
            if (v <= -2) { const int64_t t = -2 - v; v = n_rw + (remap ? m[(size_t)t] : t); }   // usum entry, library numbering
        HIPCHK(ctx->sets.d_boot_slot.upload(slot.data(), (size_t)ctx->n_rows));
        ctx->sets.boot_n_rw = n_rw;
    } catch (const std::bad_alloc &) { return EMSAR_HIP_ERR_OOM; }
    ctx->sets.boot_slot_ready = true;
    return EMSAR_HIP_OK;
}

// Swap per-row weights x (caller order) into the streaming layout, as upload_sample would place them (den and E unchanged), with the
// deterministic mode's fixed-point scales taken from their own total.  x = the sample's own weights (h_wgt) restores the sample.
int boot_stream_weights(emsar_hip_ctx *ctx, const int32_t *x) {
    LayoutWeights LW;
    double llc = 0.0;
    int rc;
    try { rc = layout_weights(ctx, [&](int64_t r) { return x[r]; }, nullptr, true, LW, llc); } catch (const std::bad_alloc &) { return EMSAR_HIP_ERR_OOM; }
    if (rc) return rc;
    set_fx_scales(ctx, std::accumulate(x, x + ctx->n_rows, (int64_t)0));
    if ((rc = upload_layout_weights(ctx, LW, true))) return rc;
    ctx->weighted = true;
    return EMSAR_HIP_OK;
}

// What a resampling call changes in the context, put back whatever the exit: finish() on the successful exit, which reports its status,
// else the destructor.
struct BootRestore {
    emsar_hip_ctx *ctx;
    bool weighted, swapped = false, finished = false;
    double fx_mass, fx_ll;
    DevBuf<double> d_th0;                  // the current point before the call
    explicit BootRestore(emsar_hip_ctx *c) : ctx(c), weighted(c->weighted), fx_mass(c->fx_mass), fx_ll(c->fx_ll) {}
    int finish() {
        if (finished) return EMSAR_HIP_OK;
        finished = true;
        int rc = EMSAR_HIP_OK;
        (void)hipStreamSynchronize(ctx->stream);
        if (swapped) {                     // the sample's own weights back; an unweighted sample has no weight arrays
            rc = boot_stream_weights(ctx, ctx->h_wgt.data());
            if (!weighted) ctx->rw = RowWeights();
            ctx->weighted = weighted;
        }
        ctx->fx_mass = fx_mass; ctx->fx_ll = fx_ll;
        if (d_th0) (void)hipMemcpy(ctx->vec.d_th[0], d_th0, (size_t)ctx->n_tx * 8, hipMemcpyDeviceToDevice);
        return rc;
    }
    ~BootRestore() { (void)finish(); }
};

// Gene sums of ncol (<= 65535) rows x[ncol][n_tx] in library order into out[ncol][n_genes], on the context's stream; part holds
// ncol * n_gene_chunks doubles (may be null when no gene has more than one chunk).
int launch_gene_sums(emsar_hip_ctx *ctx, const double *x, int64_t ncol, double *out, double *part) {
    if (ctx->genes.n_gene_chunks > 0)
        hipLaunchKernelGGL(k_gene_sums, dim3((unsigned)grid_for(ctx->genes.n_gene_chunks, 256), (unsigned)ncol), dim3(256), 0, ctx->stream,
                           ctx->genes.n_gene_chunks, ctx->genes.d_chunk_beg, ctx->genes.d_chunk_out, ctx->genes.d_gene_tx, x, (int64_t)ctx->n_tx, out,
                           (int64_t)ctx->genes.n_genes, part);
    if (ctx->genes.n_gene_multi > 0)
        hipLaunchKernelGGL(k_gene_finish, dim3((unsigned)grid_for(ctx->genes.n_gene_multi, 256), (unsigned)ncol), dim3(256), 0, ctx->stream,
                           ctx->genes.n_gene_multi, ctx->genes.d_gene_multi, part, ctx->genes.n_gene_chunks, out, (int64_t)ctx->genes.n_genes);
    HIPCHK(hipGetLastError());
    return EMSAR_HIP_OK;
}

// The dominant isoform of every gene in ncol (<= 65535) rows x[ncol][n_tx] with their gene sums gsum[ncol][n_genes] (launch_gene_sums
// before, same stream) into dom[ncol][n_genes], library indices or -1; part_v / part_i hold ncol * n_gene_chunks partials (may be
// null when no gene has more than one chunk).
int launch_iso_dominant(emsar_hip_ctx *ctx, const double *x, int64_t ncol, const double *gsum, int32_t *dom, double *part_v, int32_t *part_i) {
    if (ctx->genes.n_gene_chunks > 0)
        hipLaunchKernelGGL(k_iso_dominant, dim3((unsigned)grid_for(ctx->genes.n_gene_chunks, 256), (unsigned)ncol), dim3(256), 0, ctx->stream,
                           ctx->genes.n_gene_chunks, ctx->genes.d_chunk_beg, ctx->genes.d_chunk_out, ctx->genes.d_gene_tx, x, (int64_t)ctx->n_tx, gsum, dom,
                           (int64_t)ctx->genes.n_genes, part_v, part_i);
    if (ctx->genes.n_gene_multi > 0)
        hipLaunchKernelGGL(k_iso_dominant_finish, dim3((unsigned)grid_for(ctx->genes.n_gene_multi, 256), (unsigned)ncol), dim3(256), 0, ctx->stream,
                           ctx->genes.n_gene_multi, ctx->genes.d_gene_multi, part_v, part_i, ctx->genes.n_gene_chunks, gsum, dom, (int64_t)ctx->genes.n_genes);
    HIPCHK(hipGetLastError());
    return EMSAR_HIP_OK;
}

// What a call draws and where its results go.  fractions null: the Poisson bootstrap, one round.  Else the depth subsampling: one round
// per fraction f_k with w_c ~ Binomial(R_c, f_k), every replicate scaled to its own depth, the outputs of round k at [k][...].
// Outputs that are null are not returned; gene_mean non-null asks for the gene statistics (all null = none).
struct BootPlan {
    const double *fractions = nullptr;
    int32_t n_fractions = 1;
    double *fpkm_mean = nullptr, *fpkm_sd = nullptr, *tpm_mean = nullptr, *tpm_sd = nullptr, *replicates = nullptr;
    double *gene_mean = nullptr, *gene_sd = nullptr, *gene_tpm_mean = nullptr, *gene_tpm_sd = nullptr;
    double *depth_mean = nullptr;        // subsampling: mean over the replicates of N_b = sum_c w_c, per fraction
    // quantiles (bootstrap only, n_q > 0): every replicate's theta, S_b and gene sums stay on the device for k_boot_quantiles
    int32_t n_q = 0;
    const double *q = nullptr;
    double *fpkm_q = nullptr, *tpm_q = nullptr, *gene_fpkm_q = nullptr, *gene_tpm_q = nullptr;     // [n_q][n_tx], [n_q][n_genes]
    double *replicate_sums = nullptr;    // [n_rep] S_b
    // isoform usage (bootstrap only, needs the gene map): non-null asks for the replicates' gene sums, usage and dominant isoforms;
    // its usage_q needs n_q > 0
    const emsar_isoform_outputs *iso = nullptr;
};
struct BootTimes {
    int32_t batch = 0, unconverged = 0, passes_max = 0;
    int64_t draws = 0, held_bytes = 0;
    double draw_ms = 0, sets_ms = 0, stream_ms = 0, reduce_ms = 0, quantile_ms = 0, total_ms = 0;
};

// One resampling call: parameters, switches, sizes, buffers and counters, and the stages as functions of the batch (replicates
// done .. done + nb - 1 of the round in progress).
struct BootRun {
    emsar_hip_ctx *const ctx;
    const emsar_em_params p;             // the caller's parameters with the defaults filled in
    const uint64_t seed;
    const int32_t first, n_rep;
    const BootPlan &plan;
    // switches
    const bool genes, iso, gene_sums;    // gene statistics wanted; isoform usage wanted; either: the replicates' gene sums are needed
    const bool binomial, hold;           // binomial draws (subsampling); all replicates held on the device (quantiles)
    bool use_sets = false;               // the closed form and the resident sets, all replicates of a batch in one launch per class
    bool need_stream = false;            // a streaming solve per replicate for what the set solver does not cover
    // sizes
    const int n;                         // transcripts
    const int64_t n_rows, ng;            // rows; genes (0 when no gene sums are needed)
    const unsigned gn;                   // workgroups of a 256-thread kernel over the transcripts
    int64_t n_rw = 0, slot_stride = 0;   // row_w entries of the resident sets; one replicate's [row_w | usum] block
    int64_t n_sets = 0, n_gu = 0;        // resident sets; their transcripts, all sets together
    int64_t n_gchunk = 0, batch = 1;     // gene chunks when some gene has more than one, else 0; replicates per batch
    double n_full = 0.0;                 // subsampling: N_R, the total of the rows that are drawn
    // device buffers of the call; rows = batch, or n_rep when the replicates are held
    DevBuf<double> d_thb, d_sums, d_gsum;           // [rows][n] theta, [rows] S_b, [rows][ng] gene sums of the replicates
    DevBuf<double> d_slots, d_gu;                   // [batch][slot_stride] drawn row_w | usum of the sets, [batch][n_gu] their g_u gathered from it
    DevBuf<int32_t> d_wb;                           // [batch][n_rows] drawn weights in caller row order (streaming solves)
    DevBuf<SetStat> d_bstat;                        // [batch][n_sets]
    DevBuf<long long> d_ndrawn;                     // [batch] subsampling: N_b = sum_c w_c
    DevBuf<double> d_acc4, d_gacc4;                 // [4][n], [4][ng] Welford accumulators of transcripts and genes: FPKM mean, M2, TPM mean, M2
    DevBuf<double> d_gpart;                         // [batch][n_gchunk] chunk sums of the genes of more than one chunk
    DevBuf<double> d_q, d_qsums;                    // quantiles: [n_q] the probabilities, [n_rep] S_b added in the caller's order
    DevBuf<double> d_qout;                          // [2][n_q][n] then [2][n_q][ng]: FPKM and TPM quantiles of transcripts, then of genes
    DevBuf<int32_t> d_libof;                        // [n] caller tid -> library index, null = the same
    DevBuf<int32_t> d_dom, d_dpart_i;               // isoforms: [batch][ng] dominant isoform of the replicates' genes, [batch][n_gchunk] chunk partials
    DevBuf<double> d_dpart_v;                       // [batch][n_gchunk]
    DevBuf<double> d_uacc, d_uq;                    // [2][n] Welford accumulators of the usage; [n_q][n] its quantiles
    DevBuf<int32_t> d_ucnt;                         // [n] replicates in which the transcript is its gene's dominant isoform
    std::vector<int32_t> h_wb;           // host staging: [batch][n_rows]
    std::vector<double> h_th;            // [n] a streaming solve's result
    std::vector<SetStat> h_bstat;        // [batch][n_sets]
    std::vector<long long> h_ndrawn;     // [batch]
    std::vector<char> unconv;            // [nb] replicates of the batch with a part that hit max_iter
    int32_t fk = 0;                      // the round in progress: its index
    double frac = 1.0;                   // its fraction (1 for the bootstrap)
    long long depth_sum = 0;             // its sum of N_b
    hipEvent_t e[2] = {nullptr, nullptr};
    BootTimes t;                         // the five stage timers, unconverged, passes_max, held_bytes
    BootRestore guard;                   // last: the context is put back before the buffers above are freed

    BootRun(emsar_hip_ctx *c, const emsar_em_params &par, uint64_t seed_, int32_t first_, int32_t n_rep_, const BootPlan &plan_)
        : ctx(c), p(par), seed(seed_), first(first_), n_rep(n_rep_), plan(plan_),
          genes(plan_.gene_mean != nullptr), iso(plan_.iso != nullptr), gene_sums(genes || iso), binomial(plan_.fractions != nullptr),
          hold(plan_.n_q > 0), n(c->n_tx), n_rows(c->n_rows), ng(gene_sums ? c->genes.n_genes : 0), gn((unsigned)grid_for(c->n_tx, 256)), guard(c) {}
    ~BootRun() { for (hipEvent_t ev : e) if (ev) (void)hipEventDestroy(ev); }

    // the batch's theta, S_b and gene sums: the batch buffers, or the batch's rows of the held ones
    double *th_rows(int64_t done) const { return d_thb + (hold ? done * n : 0); }
    double *sum_rows(int64_t done) const { return d_sums + (hold ? done : 0); }
    double *gene_rows(int64_t done) const { return gene_sums ? d_gsum + (hold ? done * ng : 0) : nullptr; }
    int numeric(const char *sub, const char *boot) { ctx->err = binomial ? sub : boot; return EMSAR_HIP_ERR_NUMERIC; }
    // device time since e[0] was recorded, added to acc (the host waits for the stream)
    int lap(double &acc) {
        float ms = 0;
        HIPCHK(hipEventRecord(e[1], ctx->stream)); HIPCHK(hipEventSynchronize(e[1])); HIPCHK(hipEventElapsedTime(&ms, e[0], e[1]));
        acc += ms;
        return EMSAR_HIP_OK;
    }
    // quantiles: all n_rep replicates are held -- theta, S_b and the gene sums -- and, with the quantile stage's own buffers, must fit
    // half of the free device memory; they are allocated here, before anything is launched
    int alloc_held() {
        t.held_bytes = 8 * (int64_t)n_rep * ((int64_t)n + 1 + ng);
        const int64_t T = n, G = genes ? ng : 0, nq = plan.n_q;      // G: genes with quantile outputs
        const bool uq = iso && plan.iso->usage_q;
        const auto &m = tid_map(ctx);
        const bool remap = renumbered(ctx);
        const int64_t need = t.held_bytes + 8 * (int64_t)n_rep + 8 * nq + 16 * nq * (T + G) + (remap ? 4 * T : 0) + (uq ? 8 * nq * T : 0);
        if ((uint64_t)need > (uint64_t)(free_device_bytes() / 2)) { ctx->err = "bootstrap quantiles: the replicates do not fit half of the free device memory"; return EMSAR_HIP_ERR_OOM; }
        if (d_thb.alloc((size_t)(n_rep * T)) != hipSuccess || d_sums.alloc((size_t)n_rep) != hipSuccess || (gene_sums && d_gsum.alloc((size_t)(n_rep * ng)) != hipSuccess) || d_q.alloc((size_t)nq) != hipSuccess ||
            d_qout.alloc((size_t)(2 * nq * (T + G))) != hipSuccess || (uq && d_uq.alloc((size_t)(nq * T)) != hipSuccess) || d_qsums.alloc((size_t)n_rep) != hipSuccess || (remap && d_libof.alloc((size_t)T) != hipSuccess)) {
            (void)hipGetLastError();
            ctx->err = "bootstrap quantiles: device allocation of the held replicates failed";
            return EMSAR_HIP_ERR_OOM;
        }
        HIPCHK(hipMemcpy(d_q, plan.q, (size_t)nq * 8, hipMemcpyHostToDevice));
        if (remap) HIPCHK(hipMemcpy(d_libof, m.data(), (size_t)T * 4, hipMemcpyHostToDevice));
        return EMSAR_HIP_OK;
    }
    // which solvers run, their sizes, and the replicates per batch: what fits a quarter of the free device memory (at most 2 GiB),
    // EMSAR_HIP_BOOT_BATCH overrides
    int plan_batch() {
        int rc;
        SolvePlan sp;
        if ((rc = plan_solve(ctx, p.set_mode, sp))) return rc;
        use_sets = sp.use_sets;
        // the streaming passes solve what the set solver does not cover: everything, the streamed sets -- and here the cluster sets too
        need_stream = sp.need_stream || ctx->sets.n_cstat > 0;
        if ((rc = boot_prepare(ctx, use_sets))) return rc;
        n_rw = use_sets ? ctx->sets.boot_n_rw : 0;
        slot_stride = n_rw + n;
        n_sets = use_sets ? ctx->sets.RS.n_resident() : 0;
        if (use_sets) for (int c = 0; c < emsar::kSetClasses; c++) for (const auto &d : ctx->sets.RS.desc[c]) n_gu += d.n_t;
        n_gchunk = gene_sums && ctx->genes.n_gene_multi > 0 ? ctx->genes.n_gene_chunks : 0;
        // (a quantile call's theta, S_b and gene sums live in the held buffers, allocated before: not part of a batch, and what is free is what they left)
        const int64_t per_rep = 8 * (slot_stride + n_gu + (hold ? 0 : n + 1 + ng) + n_gchunk) + (need_stream ? 4 * n_rows : 0) + (int64_t)sizeof(SetStat) * n_sets +
                                (iso ? 4 * ng + 12 * n_gchunk : 0);
        batch = item_batch(std::max<int64_t>(per_rep, 1), "EMSAR_HIP_BOOT_BATCH", n_rep, 65535);
        return EMSAR_HIP_OK;
    }
    // the batch's device buffers (a quantile call keeps all n_rep replicates: a batch then writes its rows of the held buffers instead
    // of buffers of its own), the copy of the current point, the events, the host staging
    int allocate() {
        HIPCHK(d_slots.alloc((size_t)(batch * slot_stride))); HIPCHK(d_gu.alloc((size_t)(batch * n_gu)));
        if (!hold) { HIPCHK(d_thb.alloc((size_t)(batch * n))); HIPCHK(d_sums.alloc((size_t)batch)); }
        HIPCHK(d_acc4.alloc((size_t)(4 * (int64_t)n)));
        if (gene_sums && !hold) HIPCHK(d_gsum.alloc((size_t)(batch * ng)));
        if (n_gchunk) HIPCHK(d_gpart.alloc((size_t)(batch * n_gchunk)));
        if (iso) {
            HIPCHK(d_dom.alloc((size_t)(batch * ng)));
            if (n_gchunk) { HIPCHK(d_dpart_v.alloc((size_t)(batch * n_gchunk))); HIPCHK(d_dpart_i.alloc((size_t)(batch * n_gchunk))); }
            HIPCHK(d_uacc.alloc((size_t)(2 * (int64_t)n))); HIPCHK(d_ucnt.alloc((size_t)n));
        }
        if (genes) HIPCHK(d_gacc4.alloc((size_t)(4 * ng)));
        if (binomial) {
            HIPCHK(d_ndrawn.alloc((size_t)batch));
            h_ndrawn.resize((size_t)batch);
            n_full = (double)std::accumulate(ctx->h_wgt.begin(), ctx->h_wgt.end(), (int64_t)0);
        }
        if (need_stream) HIPCHK(d_wb.alloc((size_t)(batch * n_rows)));
        if (n_sets) HIPCHK(d_bstat.alloc((size_t)(batch * n_sets)));
        HIPCHK(guard.d_th0.alloc((size_t)n));
        HIPCHK(hipMemcpyAsync(guard.d_th0, ctx->vec.d_th[0], (size_t)n * 8, hipMemcpyDeviceToDevice, ctx->stream));
        HIPCHK(hipEventCreate(&e[0])); HIPCHK(hipEventCreate(&e[1]));
        if (n_sets) HIPCHK(set_class_lds_attributes(kSolveSetsBoot));
        h_wb.resize(need_stream ? (size_t)(batch * n_rows) : 0);
        h_th.resize((size_t)std::max(n, 1));
        h_bstat.resize((size_t)(batch * n_sets));
        return EMSAR_HIP_OK;
    }
    // the batch's weights: Poisson, or binomial at the round's fraction
    int draw(int64_t done, int64_t nb) {
        const dim3 grid((unsigned)((n_rows + 255) / 256), (unsigned)nb);
        HIPCHK(hipEventRecord(e[0], ctx->stream));
        if (use_sets) HIPCHK(hipMemsetAsync(d_slots, 0, (size_t)(nb * slot_stride) * 8, ctx->stream));
        if (binomial) HIPCHK(hipMemsetAsync(d_ndrawn, 0, (size_t)nb * 8, ctx->stream));
        if (n_rows > 0 && !binomial)
            hipLaunchKernelGGL(k_boot_draw, grid, dim3(256), 0, ctx->stream, n_rows, seed, (int64_t)first + done, ctx->sets.d_boot_R,
                               use_sets ? ctx->sets.d_boot_slot.get() : nullptr, need_stream ? d_wb.get() : nullptr, d_slots, slot_stride);
        if (n_rows > 0 && binomial)
            hipLaunchKernelGGL(k_sub_draw, grid, dim3(256), 0, ctx->stream, n_rows, seed, (int64_t)first + done, frac, ctx->sets.d_boot_R,
                               use_sets ? ctx->sets.d_boot_slot.get() : nullptr, need_stream ? d_wb.get() : nullptr, d_slots, slot_stride, d_ndrawn);
        HIPCHK(hipGetLastError());
        return lap(t.draw_ms);
    }
    // closed form + resident sets, all replicates of the batch in one launch per class
    int solve_sets(int64_t done, int64_t nb) {
        const auto &S = ctx->sets.RS;
        double *const thb = th_rows(done);
        int rc;
        HIPCHK(hipEventRecord(e[0], ctx->stream));
        if (n_gu > 0)
            hipLaunchKernelGGL(k_boot_gather_u, dim3((unsigned)((n_gu + 255) / 256), (unsigned)nb), dim3(256), 0, ctx->stream, n_gu, ctx->sets.d_g_tid,
                               d_slots, slot_stride, n_rw, d_gu);
        hipLaunchKernelGGL(k_boot_closed, dim3(gn, (unsigned)nb), dim3(256), 0, ctx->stream, n, ctx->sets.d_kind, d_slots, slot_stride, n_rw,
                           ctx->vec.d_den, thb);
        const size_t off[3] = {0, S.desc[0].size(), S.desc[0].size() + S.desc[1].size()};
        if ((rc = fork_side_streams(ctx, 2))) return rc;
        rc = launch_set_classes(ctx, 2, [&](int c, int threads, hipStream_t st) {
            hipLaunchKernelGGL(kSolveSetsBoot[c],
                               dim3((unsigned)S.desc[c].size(), (unsigned)nb), dim3(threads), S.max_lds[c], st, ctx->sets.d_sdesc[c], ctx->sets.d_g_tid, d_gu,
                               d_slots, ctx->sets.d_srp, ctx->sets.d_sent, ctx->sets.d_scp, ctx->sets.d_scrow, ctx->vec.d_den, thb, d_bstat + off[c], set_params(p), n_gu, slot_stride,
                               (int64_t)n, n_sets);
        });
        if (rc) return rc;
        if (n_sets) HIPCHK(hipMemcpyAsync(h_bstat.data(), d_bstat, (size_t)(nb * n_sets) * sizeof(SetStat), hipMemcpyDeviceToHost, ctx->stream));
        if ((rc = lap(t.sets_ms))) return rc;
        for (int64_t i = 0; i < nb * n_sets; i++) {
            const SetStat &q = h_bstat[(size_t)i];
            if (!std::isfinite(q.delta)) return numeric("non-finite theta in a connected set of a subsampling replicate", "non-finite theta in a connected set of a bootstrap replicate");
            t.passes_max = std::max(t.passes_max, q.passes);
            if (!q.converged) unconv[(size_t)(i / n_sets)] = 1;
        }
        return EMSAR_HIP_OK;
    }
    // the rest: one streaming solve per replicate with its weights swapped into the layout
    int solve_streamed(int64_t done, int64_t nb) {
        int rc;
        HIPCHK(hipMemcpyAsync(h_wb.data(), d_wb, (size_t)(nb * n_rows) * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        emsar_em_params ps = p;
        ps.set_mode = 1;
        for (int64_t y = 0; y < nb; y++) {
            guard.swapped = true;
            if ((rc = boot_stream_weights(ctx, h_wb.data() + y * n_rows))) return rc;
            emsar_em_stats st;
            if ((rc = SolveRun(ctx, &ps, h_th.data(), &st).run())) return rc;
            t.stream_ms += st.kernel_ms;
            if (!st.converged) unconv[(size_t)y] = 1;
            hipLaunchKernelGGL(k_boot_take_streamed, dim3(gn), dim3(256), 0, ctx->stream, n, use_sets ? ctx->sets.d_kind.get() : nullptr, ctx->vec.d_th[0],
                               th_rows(done) + y * n);
            HIPCHK(hipGetLastError());
        }
        return EMSAR_HIP_OK;
    }
    // reduction over the replicates, in replicate order
    int reduce(int64_t done, int64_t nb) {
        double *const thb = th_rows(done), *const sums = sum_rows(done);
        int rc;
        HIPCHK(hipEventRecord(e[0], ctx->stream));
        if (binomial)     // every replicate to its own depth: theta_b * N_R / N_b
            hipLaunchKernelGGL(k_sub_scale, dim3(gn, (unsigned)nb), dim3(256), 0, ctx->stream, n, n_full, d_ndrawn, thb);
        hipLaunchKernelGGL(k_boot_sums, dim3((unsigned)nb), dim3(1024), 0, ctx->stream, n, thb, sums);
        hipLaunchKernelGGL(k_boot_accum, dim3(gn), dim3(256), 0, ctx->stream, n, (int)nb, done, thb, sums, d_acc4);
        HIPCHK(hipGetLastError());
        if (gene_sums && (rc = launch_gene_sums(ctx, thb, nb, gene_rows(done), d_gpart))) return rc;
        if (genes) {   // the same Welford step on the replicates' gene sums (gene TPM_b = G_b * 1e6 / S_b)
            hipLaunchKernelGGL(k_boot_accum, dim3((unsigned)grid_for(ng, 256)), dim3(256), 0, ctx->stream, (int)ng, (int)nb, done, gene_rows(done), sums, d_gacc4);
            HIPCHK(hipGetLastError());
        }
        if (iso && n > 0) {   // the replicates' dominant isoforms, then usage and dominance reduced per transcript
            if ((rc = launch_iso_dominant(ctx, thb, nb, gene_rows(done), d_dom, d_dpart_v, d_dpart_i))) return rc;
            hipLaunchKernelGGL(k_iso_accum, dim3(gn), dim3(256), 0, ctx->stream, n, (int)nb, done, ctx->genes.d_gene_of_lib, thb, gene_rows(done), d_dom, ng,
                               d_uacc, d_ucnt);
            HIPCHK(hipGetLastError());
        }
        // (after the launches: a copy into pageable memory makes the host wait for the stream)
        if (binomial) HIPCHK(hipMemcpyAsync(h_ndrawn.data(), d_ndrawn, (size_t)nb * 8, hipMemcpyDeviceToHost, ctx->stream));
        if ((rc = lap(t.reduce_ms))) return rc;
        if (binomial) for (int64_t y = 0; y < nb; y++) depth_sum += h_ndrawn[(size_t)y];
        return EMSAR_HIP_OK;
    }
    // the batch's replicates into the caller's array of this round, caller numbering
    int copy_out(int64_t done, int64_t nb) {
        if (!plan.replicates) return EMSAR_HIP_OK;
        double *const replicates = plan.replicates + (int64_t)fk * n_rep * n;
        HIPCHK(hipMemcpy(replicates + done * n, th_rows(done), (size_t)(nb * n) * 8, hipMemcpyDeviceToHost));
        for (int64_t y = 0; y < nb; y++) from_lib(ctx, replicates + (done + y) * n);
        return EMSAR_HIP_OK;
    }
    // [4][cnt] accumulators to the host; the means and M2 of FPKM must be finite
    int fetch_acc(const double *d_acc, int64_t cnt, std::vector<double> &acc, const char *sub, const char *boot) {
        acc.resize((size_t)(4 * cnt));
        HIPCHK(hipMemcpyAsync(acc.data(), d_acc, acc.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        for (int64_t i = 0; i < 2 * cnt; i++) if (!std::isfinite(acc[(size_t)i])) return numeric(sub, boot);
        return EMSAR_HIP_OK;
    }
    // the round's accumulators into the caller's vectors: means and sample sd of transcripts and genes, depth_mean
    int finish_round() {
        std::vector<double> acc;
        // row r of [4][cnt] accumulators as it is (mean) or as the sample sd, into the caller's vector of this round
        auto put = [&](double *out, int r, int64_t cnt, bool sd) {
            for (int64_t i = 0; out && i < cnt; i++) {
                const double v = acc[(size_t)(r * cnt + i)];
                out[(int64_t)fk * cnt + i] = !sd ? v : n_rep > 1 ? std::sqrt(v / (double)(n_rep - 1)) : 0.0;
            }
        };
        if (int rc = fetch_acc(d_acc4, n, acc, "non-finite theta in a subsampling replicate", "non-finite theta in a bootstrap replicate")) return rc;
        double *const tx_out[4] = {plan.fpkm_mean, plan.fpkm_sd, plan.tpm_mean, plan.tpm_sd};
        for (int r = 0; r < 4; r++) { put(tx_out[r], r, n, r & 1); if (tx_out[r]) from_lib(ctx, tx_out[r] + (int64_t)fk * n); }    // caller numbering
        if (genes) {   // gene order is the caller's: no renumbering to undo
            if (int rc = fetch_acc(d_gacc4, ng, acc, "non-finite gene sum in a subsampling replicate", "non-finite gene sum in a bootstrap replicate")) return rc;
            put(plan.gene_mean, 0, ng, false); put(plan.gene_sd, 1, ng, true); put(plan.gene_tpm_mean, 2, ng, false); put(plan.gene_tpm_sd, 3, ng, true);
        }
        if (plan.depth_mean) plan.depth_mean[fk] = (double)depth_sum / (double)n_rep;
        if (iso) {   // usage is in [0, 1] whenever theta is finite, which the check above has settled
            const emsar_isoform_outputs &o = *plan.iso;
            acc.resize((size_t)(2 * (int64_t)n));
            HIPCHK(hipMemcpyAsync(acc.data(), d_uacc, acc.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
            if (o.dominant_count) HIPCHK(hipMemcpyAsync(o.dominant_count, d_ucnt, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipStreamSynchronize(ctx->stream));
            put(o.usage_mean, 0, n, false); put(o.usage_sd, 1, n, true);
            if (o.usage_mean) from_lib(ctx, o.usage_mean);
            if (o.usage_sd) from_lib(ctx, o.usage_sd);
            if (o.dominant_count) from_lib(ctx, o.dominant_count);
        }
        return EMSAR_HIP_OK;
    }
    // quantiles over the held replicates: transcripts, then genes
    int quantiles() {
        const int64_t nq = plan.n_q;
        int Bp = 1, rc;
        while (Bp < n_rep) Bp <<= 1;
        const int cs = emsar::quant_tile_shift(Bp);
        const size_t lds = ((size_t)Bp << cs) * 8;
        double *const d_gq = d_qout + 2 * nq * n;
        HIPCHK(hipEventRecord(e[0], ctx->stream));
        // S_b added in the caller's order: the TPM quantiles do not depend on the library's numbering (kernels_quant.hpp)
        hipLaunchKernelGGL(k_quant_sums, dim3((unsigned)n_rep), dim3(1024), 0, ctx->stream, n, d_libof, d_thb, d_qsums);
        if (n > 0)
            hipLaunchKernelGGL(k_boot_quantiles, dim3((unsigned)(((int64_t)n + (1 << cs) - 1) >> cs)), dim3(256), lds, ctx->stream, (int64_t)n,
                               (int)n_rep, Bp, cs, d_thb, d_qsums, (int)nq, d_q, d_qout, d_qout + nq * n);
        if (genes && ng > 0)
            hipLaunchKernelGGL(k_boot_quantiles, dim3((unsigned)((ng + (1 << cs) - 1) >> cs)), dim3(256), lds, ctx->stream, ng, (int)n_rep, Bp, cs,
                               d_gsum, d_qsums, (int)nq, d_q, d_gq, d_gq + nq * ng);
        const bool uq = iso && plan.iso->usage_q;
        if (uq && n > 0)
            hipLaunchKernelGGL(k_iso_quantiles, dim3((unsigned)(((int64_t)n + (1 << cs) - 1) >> cs)), dim3(256), lds, ctx->stream, (int64_t)n, (int)n_rep,
                               Bp, cs, ctx->genes.d_gene_of_lib, d_thb, d_gsum, ng, (int)nq, d_q, d_uq);
        HIPCHK(hipGetLastError());
        if ((rc = lap(t.quantile_ms))) return rc;
        if (uq) {
            HIPCHK(hipMemcpy(plan.iso->usage_q, d_uq, (size_t)(nq * n) * 8, hipMemcpyDeviceToHost));
            for (int64_t k = 0; k < nq; k++) from_lib(ctx, plan.iso->usage_q + k * n);
        }
        HIPCHK(hipMemcpy(plan.fpkm_q, d_qout, (size_t)(nq * n) * 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(plan.tpm_q, d_qout + nq * n, (size_t)(nq * n) * 8, hipMemcpyDeviceToHost));
        for (int64_t k = 0; k < nq; k++) { from_lib(ctx, plan.fpkm_q + k * n); from_lib(ctx, plan.tpm_q + k * n); }
        if (genes) HIPCHK(hipMemcpy(plan.gene_fpkm_q, d_gq, (size_t)(nq * ng) * 8, hipMemcpyDeviceToHost));
        if (genes) HIPCHK(hipMemcpy(plan.gene_tpm_q, d_gq + nq * ng, (size_t)(nq * ng) * 8, hipMemcpyDeviceToHost));
        if (plan.replicate_sums) HIPCHK(hipMemcpy(plan.replicate_sums, d_qsums, (size_t)n_rep * 8, hipMemcpyDeviceToHost));
        return EMSAR_HIP_OK;
    }
    int run() {
        int rc;
        if (hold && (rc = alloc_held())) return rc;
        if ((rc = plan_batch()) || (rc = allocate())) return rc;
        for (fk = 0; fk < plan.n_fractions; fk++) {
            frac = binomial ? plan.fractions[fk] : 1.0;
            depth_sum = 0;
            HIPCHK(hipMemsetAsync(d_acc4, 0, (size_t)4 * n * 8, ctx->stream));
            if (genes) HIPCHK(hipMemsetAsync(d_gacc4, 0, (size_t)4 * ng * 8, ctx->stream));
            if (iso) { HIPCHK(hipMemsetAsync(d_uacc, 0, (size_t)2 * n * 8, ctx->stream)); HIPCHK(hipMemsetAsync(d_ucnt, 0, (size_t)n * 4, ctx->stream)); }
            for (int64_t done = 0; done < n_rep; ) {
                const int64_t nb = std::min<int64_t>(batch, n_rep - done);
                unconv.assign((size_t)nb, 0);
                if ((rc = draw(done, nb)) || (use_sets && (rc = solve_sets(done, nb))) || (need_stream && (rc = solve_streamed(done, nb))) ||
                    (rc = reduce(done, nb)) || (rc = copy_out(done, nb))) return rc;
                for (char c : unconv) t.unconverged += c;
                done += nb;
            }
            if ((rc = finish_round()) || (hold && (rc = quantiles()))) return rc;
        }
        t.batch = (int32_t)batch;
        t.draws = (int64_t)std::count_if(ctx->h_wgt.begin(), ctx->h_wgt.end(), [](int32_t w) { return w > 0; }) * n_rep * plan.n_fractions;
        return guard.finish();      // the sample's own weights back before the call returns: a failure there is reported
    }
};

// one resampling call from its plan; nothing leaves it as an exception.  t is filled on success.
int run_plan(emsar_hip_ctx *ctx, const emsar_em_params *pp, uint64_t seed, int32_t first, int32_t n_rep, const BootPlan &plan, BootTimes &t) {
    const auto tw0 = std::chrono::steady_clock::now();
    try {
        const emsar_em_params p = solve_params(pp);
        if (!(p.count_floor >= 0.0) || (p.set_mode != 0 && p.set_mode != 1)) return EMSAR_HIP_ERR_ARG;
        HIPCHK(hipSetDevice(ctx->device));
        BootRun run(ctx, p, seed, first, n_rep, plan);
        const int rc = run.run();
        t = run.t;
        t.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tw0).count();
        return rc;
    } catch (const std::bad_alloc &) { return EMSAR_HIP_ERR_OOM; }
}

bool replicate_range_ok(int32_t first, int32_t n) { return n >= 1 && first >= 0 && (int64_t)first + (int64_t)n <= (int64_t)INT32_MAX + 1; }
bool sub_fraction_ok(double f) { return std::isfinite(f) && f > 0.0 && f <= 1.0; }
// isoform usage is defined on non-negative finite values
bool iso_values_ok(const double *x, int64_t cnt) { return std::all_of(x, x + cnt, [](double v) { return std::isfinite(v) && v >= 0.0; }); }
bool quantile_args_ok(int32_t n_q, const double *q) {
    return n_q >= 1 && q && std::all_of(q, q + n_q, [](double v) { return std::isfinite(v) && v >= 0.0 && v <= 1.0; });
}

// the fields emsar_boot_stats and emsar_subsample_stats share
template <class Stats> void boot_stats_out(Stats *out, const BootTimes &t, int32_t n_rep) {
    memset(out, 0, sizeof(*out));
    out->n_replicates = n_rep; out->batch = t.batch; out->replicates_unconverged = t.unconverged; out->draws = t.draws;
    out->draw_ms = t.draw_ms; out->sets_ms = t.sets_ms; out->stream_ms = t.stream_ms; out->reduce_ms = t.reduce_ms; out->total_ms = t.total_ms;
}

// a bootstrap call of any flavour: the plan run, the statistics filled on success (t_out: the times, for the caller's own statistics)
int run_bootstrap(emsar_hip_ctx *ctx, const emsar_em_params *p, uint64_t seed, int32_t first, int32_t n_rep, const BootPlan &plan, emsar_boot_stats *stats, BootTimes *t_out = nullptr) {
    BootTimes t;
    const int rc = run_plan(ctx, p, seed, first, n_rep, plan, t);
    if (rc == EMSAR_HIP_OK && stats) { boot_stats_out(stats, t, n_rep); stats->set_passes_max = t.passes_max; }
    if (t_out) *t_out = t;
    return rc;
}

// The drawn weights of one replicate, caller row order: Poisson (fraction null) or Binomial(R, *fraction).
int draw_one(emsar_hip_ctx *ctx, uint64_t seed, int32_t replicate, const double *fraction, int32_t *w_out) {
    if (!ctx || !w_out || replicate < 0 || (fraction && !sub_fraction_ok(*fraction))) return EMSAR_HIP_ERR_ARG;
    if (!ctx->have_sample) return EMSAR_HIP_ERR_STATE;
    HIPCHK(hipSetDevice(ctx->device));
    if (const int rc = boot_prepare(ctx, false)) return rc;
    if (ctx->n_rows == 0) return EMSAR_HIP_OK;
    const dim3 grid((unsigned)((ctx->n_rows + 255) / 256), 1);
    const size_t n_w = ((size_t)ctx->n_rows + 1) / 2 * 2;      // the binomial draw kernel's total, 8-byte aligned behind the weights
    DevBuf<int32_t> d_w;
    HIPCHK(d_w.alloc(fraction ? n_w + 2 : (size_t)ctx->n_rows));
    long long *d_tot = (long long *)(d_w + n_w);
    if (!fraction)
        hipLaunchKernelGGL(k_boot_draw, grid, dim3(256), 0, ctx->stream, ctx->n_rows, seed, (int64_t)replicate, ctx->sets.d_boot_R, (const int64_t *)nullptr,
                           d_w, (double *)nullptr, (int64_t)0);
    else {
        HIPCHK(hipMemsetAsync(d_tot, 0, 8, ctx->stream));
        hipLaunchKernelGGL(k_sub_draw, grid, dim3(256), 0, ctx->stream, ctx->n_rows, seed, (int64_t)replicate, *fraction, ctx->sets.d_boot_R,
                           (const int64_t *)nullptr, d_w, (double *)nullptr, (int64_t)0, d_tot);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(w_out, d_w, (size_t)ctx->n_rows * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return EMSAR_HIP_OK;
}

}  // namespace

extern "C" {

// ---- bootstrap --------------------------------------------------------------------------------------------------------------
int emsar_hip_bootstrap(emsar_hip_ctx *ctx, const emsar_em_params *p, uint64_t seed, int32_t first_replicate, int32_t n_replicates,
                        double *fpkm_mean, double *fpkm_sd, double *tpm_sd, double *replicates, emsar_boot_stats *stats) {
    if (!ctx) return EMSAR_HIP_ERR_ARG;
    if (!ctx->have_sample) return EMSAR_HIP_ERR_STATE;
    if (!fpkm_mean || !fpkm_sd || !tpm_sd || !replicate_range_ok(first_replicate, n_replicates)) return EMSAR_HIP_ERR_ARG;
    BootPlan plan;
    plan.fpkm_mean = fpkm_mean; plan.fpkm_sd = fpkm_sd; plan.tpm_sd = tpm_sd; plan.replicates = replicates;
    return run_bootstrap(ctx, p, seed, first_replicate, n_replicates, plan, stats);
}

int emsar_hip_bootstrap_genes(emsar_hip_ctx *ctx, const emsar_em_params *p, uint64_t seed, int32_t first_replicate, int32_t n_replicates,
                              double *fpkm_mean, double *fpkm_sd, double *tpm_sd, double *replicates,
                              double *gene_fpkm_mean, double *gene_fpkm_sd, double *gene_tpm_sd, emsar_boot_stats *stats) {
    if (!ctx) return EMSAR_HIP_ERR_ARG;
    if (!ctx->have_sample || !ctx->genes.have_genes) return EMSAR_HIP_ERR_STATE;
    if (!fpkm_mean || !fpkm_sd || !tpm_sd || !gene_fpkm_mean || !gene_fpkm_sd || !gene_tpm_sd || !replicate_range_ok(first_replicate, n_replicates)) return EMSAR_HIP_ERR_ARG;
    BootPlan plan;
    plan.fpkm_mean = fpkm_mean; plan.fpkm_sd = fpkm_sd; plan.tpm_sd = tpm_sd; plan.replicates = replicates;
    plan.gene_mean = gene_fpkm_mean; plan.gene_sd = gene_fpkm_sd; plan.gene_tpm_sd = gene_tpm_sd;
    return run_bootstrap(ctx, p, seed, first_replicate, n_replicates, plan, stats);
}

// ---- bootstrap quantiles ------------------------------------------------------------------------------------------------------
int emsar_hip_bootstrap_quantiles(emsar_hip_ctx *ctx, const emsar_em_params *p, uint64_t seed, int32_t first_replicate, int32_t n_replicates,
                                  int32_t n_q, const double *q, double *fpkm_mean, double *fpkm_sd, double *tpm_sd, double *replicates,
                                  double *replicate_sums, double *fpkm_q, double *tpm_q, double *gene_fpkm_mean, double *gene_fpkm_sd,
                                  double *gene_tpm_sd, double *gene_fpkm_q, double *gene_tpm_q, emsar_boot_stats *stats,
                                  emsar_quantile_stats *qstats) {
    if (!ctx) return EMSAR_HIP_ERR_ARG;
    if (!ctx->have_sample) return EMSAR_HIP_ERR_STATE;
    const int n_gene_out = (gene_fpkm_mean != nullptr) + (gene_fpkm_sd != nullptr) + (gene_tpm_sd != nullptr) + (gene_fpkm_q != nullptr) +
                           (gene_tpm_q != nullptr);
    if (!fpkm_mean || !fpkm_sd || !tpm_sd || !fpkm_q || !tpm_q || n_replicates > emsar::kQuantMaxRep || !replicate_range_ok(first_replicate, n_replicates) ||
        !quantile_args_ok(n_q, q) || (n_gene_out != 0 && n_gene_out != 5))
        return EMSAR_HIP_ERR_ARG;
    if (n_gene_out && !ctx->genes.have_genes) return EMSAR_HIP_ERR_STATE;
    BootPlan plan;
    plan.fpkm_mean = fpkm_mean; plan.fpkm_sd = fpkm_sd; plan.tpm_sd = tpm_sd; plan.replicates = replicates;
    plan.gene_mean = gene_fpkm_mean; plan.gene_sd = gene_fpkm_sd; plan.gene_tpm_sd = gene_tpm_sd;
    plan.n_q = n_q; plan.q = q; plan.fpkm_q = fpkm_q; plan.tpm_q = tpm_q; plan.gene_fpkm_q = gene_fpkm_q; plan.gene_tpm_q = gene_tpm_q; plan.replicate_sums = replicate_sums;
    BootTimes t;
    const int rc = run_bootstrap(ctx, p, seed, first_replicate, n_replicates, plan, stats, &t);
    if (rc == EMSAR_HIP_OK && qstats) { memset(qstats, 0, sizeof(*qstats)); qstats->n_quantiles = n_q; qstats->held_bytes = t.held_bytes; qstats->quantile_ms = t.quantile_ms; }
    return rc;
}

int emsar_hip_quantiles_host(int32_t n_rep, int64_t n, const double *values, int32_t n_q, const double *q, double *out) {
    if (n_rep < 1 || n < 0 || (n > 0 && (!values || !out)) || !quantile_args_ok(n_q, q)) return EMSAR_HIP_ERR_ARG;
    try {
        std::vector<double> col((size_t)n_rep);
        for (int64_t t = 0; t < n; t++) {
            for (int32_t b = 0; b < n_rep; b++) col[(size_t)b] = values[(int64_t)b * n + t];
            std::sort(col.begin(), col.end(), [](double a, double b) { return a < b || (b != b && a == a); });   // NaN last: a strict weak order
            for (int32_t k = 0; k < n_q; k++) out[(int64_t)k * n + t] = emsar::quantile_sorted(col.data(), 1, n_rep, q[k]);
        }
    } catch (const std::bad_alloc &) { return EMSAR_HIP_ERR_OOM; }
    return EMSAR_HIP_OK;
}

// ---- gene map -----------------------------------------------------------------------------------------------------------------
int emsar_hip_set_gene_map(emsar_hip_ctx *ctx, int32_t n_genes, const int32_t *gene_of_tx) {
    if (!ctx) return EMSAR_HIP_ERR_ARG;
    if (!ctx->have_structure) return EMSAR_HIP_ERR_STATE;
    if (n_genes < 1 || (!gene_of_tx && ctx->n_tx > 0)) return EMSAR_HIP_ERR_ARG;
    const int32_t n = ctx->n_tx;
    for (int32_t t = 0; t < n; t++) if (gene_of_tx[t] < -1 || gene_of_tx[t] >= n_genes) return EMSAR_HIP_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->genes = GeneMap();
    try {
        // gene CSR in library indices, each gene's transcripts by ascending caller tid; then its chunks of kGeneChunk
        std::vector<int64_t> gp((size_t)n_genes + 1, 0);
        for (int32_t t = 0; t < n; t++) if (gene_of_tx[t] >= 0) gp[(size_t)gene_of_tx[t] + 1]++;
        for (int32_t g = 0; g < n_genes; g++) gp[(size_t)g + 1] += gp[(size_t)g];
        const int64_t m = gp[(size_t)n_genes];
        std::vector<int32_t> tx((size_t)m), chunk_beg, chunk_out, multi, of_lib((size_t)n);
        std::vector<int64_t> fill(gp.begin(), gp.end() - 1);
        const auto &map = tid_map(ctx);
        const bool remap = renumbered(ctx);
        for (int32_t t = 0; t < n; t++)
            if (gene_of_tx[t] >= 0) tx[(size_t)fill[(size_t)gene_of_tx[t]]++] = remap ? map[(size_t)t] : t;
        for (int32_t t = 0; t < n; t++) of_lib[(size_t)(remap ? map[(size_t)t] : t)] = gene_of_tx[t];
        for (int32_t g = 0; g < n_genes; g++) {
            const int64_t len = gp[(size_t)g + 1] - gp[(size_t)g];
            const int64_t nch = std::max<int64_t>(1, (len + kGeneChunk - 1) / kGeneChunk);     // an empty gene: one empty chunk, sum 0
            if (nch > 1) { multi.push_back(g); multi.push_back((int32_t)chunk_out.size()); multi.push_back((int32_t)(chunk_out.size() + nch)); }
            for (int64_t j = 0; j < nch; j++) {
                chunk_beg.push_back((int32_t)(gp[(size_t)g] + j * kGeneChunk));
                chunk_out.push_back(nch == 1 ? g : -1);
            }
            if (chunk_out.size() > (size_t)INT32_MAX - 1) return EMSAR_HIP_ERR_ARG;
        }
        chunk_beg.push_back((int32_t)m);
        const size_t nc = chunk_out.size();
        std::vector<int32_t> blk;
        blk.reserve((size_t)m + 2 * nc + 1 + multi.size() + (size_t)n);
        blk.insert(blk.end(), tx.begin(), tx.end());
        blk.insert(blk.end(), chunk_beg.begin(), chunk_beg.end());
        blk.insert(blk.end(), chunk_out.begin(), chunk_out.end());
        blk.insert(blk.end(), multi.begin(), multi.end());
        blk.insert(blk.end(), of_lib.begin(), of_lib.end());
        GeneMap G;                   // moved into the context when it is complete
        HIPCHK(G.d_gene_blk.upload(blk.data(), blk.size()));
        G.d_gene_tx = G.d_gene_blk;
        G.d_chunk_beg = G.d_gene_tx + m;
        G.d_chunk_out = G.d_chunk_beg + nc + 1;
        G.d_gene_multi = G.d_chunk_out + nc;
        G.d_gene_of_lib = G.d_gene_multi + multi.size();
        G.n_genes = n_genes; G.n_gene_chunks = (int64_t)nc; G.n_gene_multi = (int64_t)multi.size() / 3;
        G.h_gene_of_tx.assign(gene_of_tx, gene_of_tx + n);
        G.have_genes = true;
        ctx->genes = std::move(G);
    } catch (const std::bad_alloc &) { return EMSAR_HIP_ERR_OOM; }
    return EMSAR_HIP_OK;
}

int emsar_hip_gene_sums(emsar_hip_ctx *ctx, int32_t n_cols, const double *tx_values, double *gene_out) {
    if (!ctx) return EMSAR_HIP_ERR_ARG;
    if (!ctx->have_structure || !ctx->genes.have_genes) return EMSAR_HIP_ERR_STATE;
    if (n_cols < 1 || !tx_values || !gene_out) return EMSAR_HIP_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    const int64_t n = ctx->n_tx, ng = ctx->genes.n_genes, nc = ctx->genes.n_gene_multi > 0 ? ctx->genes.n_gene_chunks : 0;
    const int64_t cb = std::min<int64_t>(n_cols, 65535);        // columns per launch (grid y)
    DevBuf<double> d_x, d_out, d_part;
    HIPCHK(d_x.alloc((size_t)(cb * n)));
    HIPCHK(d_out.alloc((size_t)(cb * ng)));
    if (nc) HIPCHK(d_part.alloc((size_t)(cb * nc)));
    try {
        std::vector<double> tmp;
        for (int64_t c0 = 0; c0 < n_cols; c0 += cb) {
            const int64_t k = std::min<int64_t>(cb, n_cols - c0);
            for (int64_t j = 0; j < k; j++) {
                const double *col = to_lib(ctx, tx_values + (c0 + j) * n, tmp);
                HIPCHK(hipMemcpy(d_x + j * n, col, (size_t)n * 8, hipMemcpyHostToDevice));
            }
            int rc = launch_gene_sums(ctx, d_x, k, d_out, d_part);
            if (rc) return rc;
            HIPCHK(hipMemcpyAsync(gene_out + c0 * ng, d_out, (size_t)(k * ng) * 8, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipStreamSynchronize(ctx->stream));
        }
    } catch (const std::bad_alloc &) { return EMSAR_HIP_ERR_OOM; }
    return EMSAR_HIP_OK;
}

// ---- isoform usage --------------------------------------------------------------------------------------------------------------
int emsar_hip_isoform_usage(emsar_hip_ctx *ctx, int32_t n_cols, const double *tx_values, double *usage_out, int32_t *dominant_out) {
    if (!ctx) return EMSAR_HIP_ERR_ARG;
    if (!ctx->have_structure || !ctx->genes.have_genes) return EMSAR_HIP_ERR_STATE;
    if (n_cols < 1 || !tx_values || !usage_out) return EMSAR_HIP_ERR_ARG;
    const int64_t n = ctx->n_tx, ng = ctx->genes.n_genes, nc = ctx->genes.n_gene_multi > 0 ? ctx->genes.n_gene_chunks : 0;
    if (!iso_values_ok(tx_values, (int64_t)n_cols * n)) return EMSAR_HIP_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    const int64_t cb = std::min<int64_t>(n_cols, 65535);        // columns per launch (grid y)
    DevBuf<double> d_x, d_gs, d_part, d_u, d_pv;
    DevBuf<int32_t> d_dom, d_pi;
    HIPCHK(d_x.alloc((size_t)(cb * n)));
    HIPCHK(d_gs.alloc((size_t)(cb * ng)));
    HIPCHK(d_u.alloc((size_t)(cb * n)));
    if (nc) HIPCHK(d_part.alloc((size_t)(cb * nc)));
    if (dominant_out) {
        HIPCHK(d_dom.alloc((size_t)(cb * ng)));
        if (nc) { HIPCHK(d_pv.alloc((size_t)(cb * nc))); HIPCHK(d_pi.alloc((size_t)(cb * nc))); }
    }
    try {
        std::vector<double> tmp;
        const std::vector<int32_t> caller_of = dominant_out ? caller_of_lib(ctx) : std::vector<int32_t>();      // library index -> caller tid, empty = the same
        for (int64_t c0 = 0; c0 < n_cols; c0 += cb) {
            const int64_t k = std::min<int64_t>(cb, n_cols - c0);
            for (int64_t j = 0; j < k; j++) {
                const double *col = to_lib(ctx, tx_values + (c0 + j) * n, tmp);
                HIPCHK(hipMemcpy(d_x + j * n, col, (size_t)n * 8, hipMemcpyHostToDevice));
            }
            int rc = launch_gene_sums(ctx, d_x, k, d_gs, d_part);
            if (rc) return rc;
            if (n > 0)
                hipLaunchKernelGGL(k_iso_usage, dim3((unsigned)grid_for(n, 256), (unsigned)k), dim3(256), 0, ctx->stream, (int)n, ctx->genes.d_gene_of_lib,
                                   d_x, d_gs, ng, d_u);
            HIPCHK(hipGetLastError());
            if (dominant_out && (rc = launch_iso_dominant(ctx, d_x, k, d_gs, d_dom, d_pv, d_pi))) return rc;
            HIPCHK(hipMemcpyAsync(usage_out + c0 * n, d_u, (size_t)(k * n) * 8, hipMemcpyDeviceToHost, ctx->stream));
            if (dominant_out) HIPCHK(hipMemcpyAsync(dominant_out + c0 * ng, d_dom, (size_t)(k * ng) * 4, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipStreamSynchronize(ctx->stream));
            for (int64_t j = 0; j < k; j++) from_lib(ctx, usage_out + (c0 + j) * n);
            if (!caller_of.empty())
                for (int64_t i = c0 * ng; i < (c0 + k) * ng; i++) if (dominant_out[i] >= 0) dominant_out[i] = caller_of[(size_t)dominant_out[i]];
        }
    } catch (const std::bad_alloc &) { return EMSAR_HIP_ERR_OOM; }
    return EMSAR_HIP_OK;
}

int emsar_hip_isoform_usage_host(int32_t n_tx, int32_t n_genes, const int32_t *gene_of_tx, int32_t n_cols, const double *tx_values,
                                 double *usage_out, int32_t *dominant_out) {
    if (n_tx < 0 || n_genes < 1 || (!gene_of_tx && n_tx > 0) || n_cols < 1 || (n_tx > 0 && (!tx_values || !usage_out))) return EMSAR_HIP_ERR_ARG;
    for (int32_t t = 0; t < n_tx; t++) if (gene_of_tx[t] < -1 || gene_of_tx[t] >= n_genes) return EMSAR_HIP_ERR_ARG;
    if (!iso_values_ok(tx_values, (int64_t)n_cols * n_tx)) return EMSAR_HIP_ERR_ARG;
    try {
        // gene CSR by ascending tid, as set_gene_map builds it
        std::vector<int64_t> gp((size_t)n_genes + 1, 0);
        for (int32_t t = 0; t < n_tx; t++) if (gene_of_tx[t] >= 0) gp[(size_t)gene_of_tx[t] + 1]++;
        for (int32_t g = 0; g < n_genes; g++) gp[(size_t)g + 1] += gp[(size_t)g];
        std::vector<int32_t> tx((size_t)gp[(size_t)n_genes]);
        std::vector<int64_t> fill(gp.begin(), gp.end() - 1);
        for (int32_t t = 0; t < n_tx; t++) if (gene_of_tx[t] >= 0) tx[(size_t)fill[(size_t)gene_of_tx[t]]++] = t;
        std::vector<double> gs((size_t)n_genes);
        for (int32_t c = 0; c < n_cols; c++) {
            const double *x = tx_values + (int64_t)c * n_tx;
            for (int32_t g = 0; g < n_genes; g++) {
                // chunks of kGeneChunk added left to right, then the chunk sums left to right; the first maximum by a strict >
                double sum = 0.0, best = 0.0;
                int32_t at = -1;
                for (int64_t b = gp[(size_t)g]; b < gp[(size_t)g + 1]; b += kGeneChunk) {
                    const int64_t e = std::min<int64_t>(b + kGeneChunk, gp[(size_t)g + 1]);
                    double s = x[tx[(size_t)b]];
                    for (int64_t i = b + 1; i < e; i++) s += x[tx[(size_t)i]];
                    sum = b == gp[(size_t)g] ? s : sum + s;
                    for (int64_t i = b; i < e; i++) if (at < 0 || x[tx[(size_t)i]] > best) { best = x[tx[(size_t)i]]; at = tx[(size_t)i]; }
                }
                gs[(size_t)g] = sum;
                if (dominant_out) dominant_out[(int64_t)c * n_genes + g] = sum > 0.0 ? at : -1;
            }
            for (int32_t t = 0; t < n_tx; t++)
                usage_out[(int64_t)c * n_tx + t] = gene_of_tx[t] >= 0 ? emsar::iso_usage(x[t], gs[(size_t)gene_of_tx[t]]) : 0.0;
        }
    } catch (const std::bad_alloc &) { return EMSAR_HIP_ERR_OOM; }
    return EMSAR_HIP_OK;
}

int emsar_hip_bootstrap_isoforms(emsar_hip_ctx *ctx, const emsar_em_params *p, uint64_t seed, int32_t first_replicate, int32_t n_replicates,
                                 int32_t n_q, const double *q, double *fpkm_mean, double *fpkm_sd, double *tpm_sd, double *replicates,
                                 double *replicate_sums, double *fpkm_q, double *tpm_q, double *gene_fpkm_mean, double *gene_fpkm_sd,
                                 double *gene_tpm_sd, double *gene_fpkm_q, double *gene_tpm_q, emsar_boot_stats *stats,
                                 emsar_quantile_stats *qstats, const emsar_isoform_outputs *iso) {
    if (!ctx) return EMSAR_HIP_ERR_ARG;
    if (!ctx->have_sample || !ctx->genes.have_genes) return EMSAR_HIP_ERR_STATE;
    if (!iso || n_q < 0 || !fpkm_mean || !fpkm_sd || !tpm_sd || !replicate_range_ok(first_replicate, n_replicates)) return EMSAR_HIP_ERR_ARG;
    const int n_gene_stat = (gene_fpkm_mean != nullptr) + (gene_fpkm_sd != nullptr) + (gene_tpm_sd != nullptr);
    BootPlan plan;
    if (n_q == 0) {      // no quantiles: nothing is held, q and the quantile outputs are not looked at
        if (iso->usage_q || (n_gene_stat != 0 && n_gene_stat != 3)) return EMSAR_HIP_ERR_ARG;
    } else {
        const int n_gene_out = n_gene_stat + (gene_fpkm_q != nullptr) + (gene_tpm_q != nullptr);
        if (!fpkm_q || !tpm_q || n_replicates > emsar::kQuantMaxRep || !quantile_args_ok(n_q, q) || (n_gene_out != 0 && n_gene_out != 5)) return EMSAR_HIP_ERR_ARG;
        plan.n_q = n_q; plan.q = q; plan.fpkm_q = fpkm_q; plan.tpm_q = tpm_q; plan.gene_fpkm_q = gene_fpkm_q; plan.gene_tpm_q = gene_tpm_q; plan.replicate_sums = replicate_sums;
    }
    plan.fpkm_mean = fpkm_mean; plan.fpkm_sd = fpkm_sd; plan.tpm_sd = tpm_sd; plan.replicates = replicates;
    plan.gene_mean = gene_fpkm_mean; plan.gene_sd = gene_fpkm_sd; plan.gene_tpm_sd = gene_tpm_sd;
    plan.iso = iso;
    BootTimes t;
    const int rc = run_bootstrap(ctx, p, seed, first_replicate, n_replicates, plan, stats, &t);
    if (rc == EMSAR_HIP_OK && qstats) { memset(qstats, 0, sizeof(*qstats)); qstats->n_quantiles = n_q; qstats->held_bytes = t.held_bytes; qstats->quantile_ms = t.quantile_ms; }
    return rc;
}

int emsar_hip_bootstrap_weights(emsar_hip_ctx *ctx, uint64_t seed, int32_t replicate, int32_t *w_out) { return draw_one(ctx, seed, replicate, nullptr, w_out); }
int emsar_hip_bootstrap_draw_host(uint64_t seed, int32_t replicate, int64_t n_rows, const int32_t *row_weight, int32_t *w_out) {
    if (replicate < 0 || n_rows < 0 || (n_rows > 0 && !w_out)) return EMSAR_HIP_ERR_ARG;
    if (row_weight) for (int64_t r = 0; r < n_rows; r++) if (row_weight[r] < 0) return EMSAR_HIP_ERR_ARG;
    for (int64_t r = 0; r < n_rows; r++) w_out[r] = emsar::boot_poisson(seed, (uint64_t)replicate, (uint64_t)r, row_weight ? row_weight[r] : 1);
    return EMSAR_HIP_OK;
}

// ---- depth subsampling ----------------------------------------------------------------------------------------------------------
int emsar_hip_subsample(emsar_hip_ctx *ctx, const emsar_em_params *p, uint64_t seed, int32_t n_fractions, const double *fractions,
                        int32_t n_replicates, double *fpkm_mean, double *fpkm_sd, double *tpm_mean, double *tpm_sd, double *depth_mean,
                        double *replicates, double *gene_fpkm_mean, double *gene_fpkm_sd, double *gene_tpm_mean, emsar_subsample_stats *stats) {
    if (!ctx) return EMSAR_HIP_ERR_ARG;
    if (!ctx->have_sample) return EMSAR_HIP_ERR_STATE;
    if (n_fractions < 1 || !fractions || !replicate_range_ok(0, n_replicates) || !fpkm_mean || !fpkm_sd || !tpm_mean || !tpm_sd || !depth_mean) return EMSAR_HIP_ERR_ARG;
    for (int32_t k = 0; k < n_fractions; k++) if (!sub_fraction_ok(fractions[k])) return EMSAR_HIP_ERR_ARG;
    const int n_gene_out = (gene_fpkm_mean != nullptr) + (gene_fpkm_sd != nullptr) + (gene_tpm_mean != nullptr);
    if (n_gene_out != 0 && n_gene_out != 3) return EMSAR_HIP_ERR_ARG;
    if (n_gene_out && !ctx->genes.have_genes) return EMSAR_HIP_ERR_STATE;
    BootPlan plan;
    plan.fractions = fractions; plan.n_fractions = n_fractions;
    plan.fpkm_mean = fpkm_mean; plan.fpkm_sd = fpkm_sd; plan.tpm_mean = tpm_mean; plan.tpm_sd = tpm_sd; plan.replicates = replicates;
    plan.gene_mean = gene_fpkm_mean; plan.gene_sd = gene_fpkm_sd; plan.gene_tpm_mean = gene_tpm_mean;
    plan.depth_mean = depth_mean;
    BootTimes t;
    const int rc = run_plan(ctx, p, seed, 0, n_replicates, plan, t);
    if (rc == EMSAR_HIP_OK && stats) { boot_stats_out(stats, t, n_replicates); stats->n_fractions = n_fractions; }
    return rc;
}

int emsar_hip_subsample_weights(emsar_hip_ctx *ctx, uint64_t seed, int32_t replicate, double fraction, int32_t *w_out) { return draw_one(ctx, seed, replicate, &fraction, w_out); }
int emsar_hip_subsample_draw_host(uint64_t seed, int32_t replicate, double fraction, int64_t n_rows, const int32_t *row_weight, int32_t *w_out) {
    if (replicate < 0 || n_rows < 0 || (n_rows > 0 && !w_out) || !sub_fraction_ok(fraction)) return EMSAR_HIP_ERR_ARG;
    if (row_weight) for (int64_t r = 0; r < n_rows; r++) if (row_weight[r] < 0) return EMSAR_HIP_ERR_ARG;
    for (int64_t r = 0; r < n_rows; r++)
        w_out[r] = emsar::boot_binomial(seed, (uint64_t)replicate, (uint64_t)r, row_weight ? row_weight[r] : 1, fraction);
    return EMSAR_HIP_OK;
}

}  // extern "C"
