// solve.hpp -- the solve driver behind emsar_hip_solve and emsar_hip_run_passes, and the set solver's driver.  Part of emsar_hip.hip's
// translation unit, included after its ABI of uploads and before resample.hpp: it uses the context, launch_pass (pass_launch.hpp),
// host_ll and the kernels (kernels_vector.hpp, kernels_sets.hpp, kernels_cluster.hpp).
// One solve = one SolveRun:  plan (parameters, sets / no sets / giant set, the rules of a pass)
//                            stream: cycles of the streaming passes, one by one or replayed from a hipGraph; poll the stopping rule
//                            resident sets (closed form, size classes, clusters) and their statistics' copies
//                            likelihood pass at the returned point, fetch
//                            collect the sets' statistics; fill emsar_em_stats
// Nothing of a solve stays in the context: what a pass needs beyond its vectors travels as a PassRules value.

namespace {

// ---- the set driver: the sample's connected sets on the device, and their launches ------------------------------------------------

// the dynamic LDS that the three size classes of a set-kernel family may ask for (the families: SetKernels, kernels_sets.hpp)
template <class Kernel> hipError_t set_class_lds_attributes(const SetKernels<Kernel> &family) {
    for (int c = 0; c < emsar::kSetClasses; c++)
        if (const hipError_t e = hipFuncSetAttribute((const void *)family[c], hipFuncAttributeMaxDynamicSharedMemorySize, (int)emsar::kSetLdsCap[c])) return e;
    return hipSuccess;
}

// the sets were found on the caller's CSR; theta / den on the device are in the library's numbering
int renumber_sets(const emsar_hip_ctx *ctx, emsar::ResidentSets &S) {
    if (!renumbered(ctx)) return EMSAR_HIP_OK;
    const auto &m = tid_map(ctx);
    try {
        std::vector<uint8_t> kind(S.kind.size());
        std::vector<double> usum(S.usum.size());
        for (size_t t = 0; t < m.size(); t++) { kind[(size_t)m[t]] = S.kind[t]; usum[(size_t)m[t]] = S.usum[t]; }
        S.kind.swap(kind); S.usum.swap(usum);
    } catch (const std::bad_alloc &) { return EMSAR_HIP_ERR_OOM; }
    for (int32_t &t : S.g_tid) t = m[(size_t)t];
    for (int32_t &t : S.CL.g_tid) t = m[(size_t)t];
    return EMSAR_HIP_OK;
}

// the records of the LDS-resident sets; the device copies are the only ones needed afterwards (desc sizes and counters stay)
int upload_resident_records(emsar_hip_ctx *ctx, emsar::ResidentSets &S) {
    SetsDev &D = ctx->sets;
    const int64_t n = S.n_resident();
    if (n > 0) {
        HIPCHK(D.d_g_tid.upload(S.g_tid.data(), S.g_tid.size()));
        HIPCHK(D.d_g_u.upload(S.g_u.data(), S.g_u.size()));
        HIPCHK(D.d_row_w.upload(S.row_w.data(), S.row_w.size()));
        HIPCHK(D.d_srp.upload(S.rp.data(), S.rp.size()));
        HIPCHK(D.d_sent.upload(S.ent.data(), S.ent.size()));
        HIPCHK(D.d_scp.upload(S.cp.data(), S.cp.size()));
        HIPCHK(D.d_scrow.upload(S.crow.data(), S.crow.size()));
        for (int c = 0; c < emsar::kSetClasses; c++)
            if (!S.desc[c].empty()) HIPCHK(D.d_sdesc[c].upload(S.desc[c].data(), S.desc[c].size()));
        HIPCHK(D.d_sstat.alloc((size_t)n));
        HIPCHK(D.h_sstat.alloc((size_t)n));
        D.n_sstat = n;
        HIPCHK(set_class_lds_attributes(kSolveSets));
    }
    std::vector<int32_t>().swap(S.g_tid); std::vector<double>().swap(S.g_u); std::vector<double>().swap(S.row_w);
    std::vector<uint16_t>().swap(S.rp); std::vector<uint16_t>().swap(S.ent); std::vector<uint16_t>().swap(S.cp); std::vector<uint16_t>().swap(S.crow);
    return EMSAR_HIP_OK;
}

// the records of the workgroup-cluster sets; only the sizes are needed afterwards
int upload_cluster_records(emsar_hip_ctx *ctx, emsar::ResidentSets &S) {
    SetsDev &D = ctx->sets;
    const int64_t nc = S.n_cluster_sets();
    if (nc == 0) return EMSAR_HIP_OK;
    auto &CL = S.CL;
    HIPCHK(D.d_cdesc.upload(CL.desc.data(), CL.desc.size()));
    HIPCHK(D.d_cblk.upload(CL.blk_set.data(), CL.blk_set.size()));
    HIPCHK(D.d_crp.upload(CL.rp.data(), CL.rp.size()));
    HIPCHK(D.d_ccp.upload(CL.cp.data(), CL.cp.size()));
    HIPCHK(D.d_cpart.upload(CL.part.data(), CL.part.size()));
    HIPCHK(D.d_cent.upload(CL.ent.data(), CL.ent.size()));
    HIPCHK(D.d_ccrow.upload(CL.crow.data(), CL.crow.size()));
    HIPCHK(D.d_cg_tid.upload(CL.g_tid.data(), CL.g_tid.size()));
    HIPCHK(D.d_cg_u.upload(CL.g_u.data(), CL.g_u.size()));
    HIPCHK(D.d_crow_w.upload(CL.row_w.data(), CL.row_w.size()));
    HIPCHK(D.d_cscratch.alloc((size_t)CL.scratch_doubles));
    HIPCHK(D.d_cbar.alloc((size_t)nc * 2));
    HIPCHK(D.d_cstat.alloc((size_t)nc));
    HIPCHK(D.h_cstat.alloc((size_t)nc));
    D.n_cstat = nc;
    HIPCHK(hipFuncSetAttribute((const void *)k_solve_cluster, hipFuncAttributeMaxDynamicSharedMemorySize, (int)emsar::kClusterLdsCap));
    std::vector<uint32_t>().swap(CL.rp); std::vector<uint32_t>().swap(CL.cp); std::vector<uint16_t>().swap(CL.ent); std::vector<uint16_t>().swap(CL.crow);
    std::vector<int32_t>().swap(CL.g_tid); std::vector<double>().swap(CL.g_u); std::vector<double>().swap(CL.row_w);
    return EMSAR_HIP_OK;
}

// find and pack the connected sets of the current sample (sets.hpp) and move the records to the device
int ensure_sets_impl(emsar_hip_ctx *ctx) {
    const auto t0 = std::chrono::steady_clock::now();
    auto &S = ctx->sets.RS;
    int rc;
    try {
        emsar::build_sets(ctx->n_rows, ctx->n_tx, ctx->h_row_ptr.data(), ctx->h_col.data(), ctx->h_wgt.data(), S);
    } catch (const std::bad_alloc &) { return EMSAR_HIP_ERR_OOM; }
    if ((rc = renumber_sets(ctx, S))) return rc;
    HIPCHK(ctx->sets.d_kind.upload(S.kind.data(), S.kind.size()));
    HIPCHK(ctx->sets.d_usum.upload(S.usum.data(), S.usum.size()));
    std::vector<double>().swap(S.usum);
    if ((rc = upload_resident_records(ctx, S)) || (rc = upload_cluster_records(ctx, S))) return rc;
    ctx->sets_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    ctx->sets.sets_ready = true;
    return EMSAR_HIP_OK;
}
int ensure_sets(emsar_hip_ctx *ctx) {
    if (ctx->sets.sets_ready) return EMSAR_HIP_OK;
    const int rc = ensure_sets_impl(ctx);
    if (rc != EMSAR_HIP_OK) ctx->sets = SetsDev();       // a half-uploaded record set is freed, the next solve starts over
    return rc;
}

// The three size classes of the set solver are independent (disjoint sets, disjoint theta entries): the larger two run on side streams next to
// the 64-thread class.  fork_side_streams: the first n_side side streams wait for ctx->stream; launch_set_classes: launch(class, threads,
// stream) for every class that has sets, the big ones first (the fewest, the longest per pass), then ctx->stream waits for those side streams.
int fork_side_streams(emsar_hip_ctx *ctx, int n_side) {
    HIPCHK(hipEventRecord(ctx->ev_fork, ctx->stream));
    for (int i = 0; i < n_side; i++) HIPCHK(hipStreamWaitEvent(ctx->side[i], ctx->ev_fork, 0));
    return EMSAR_HIP_OK;
}
template <class Launch>
int launch_set_classes(emsar_hip_ctx *ctx, int n_side, const Launch &launch) {
    const hipStream_t st[emsar::kSetClasses] = {ctx->stream, ctx->side[0], ctx->side[1]};
    for (int c = emsar::kSetClasses - 1; c >= 0; c--) if (!ctx->sets.RS.desc[c].empty()) launch(c, emsar::kSetThreads[c], st[c]);
    for (int i = 0; i < n_side; i++) {
        HIPCHK(hipEventRecord(ctx->ev_join[i], ctx->side[i]));
        HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->ev_join[i], 0));
    }
    HIPCHK(hipGetLastError());
    return EMSAR_HIP_OK;
}

// The clusters, on a stream of their own (side[2], forked before).  Every workgroup of a launch must be resident at once (they wait for
// each other at the cluster barriers): at most one workgroup per CU per launch -- each asks for most of a CU's LDS --, whole sets only.
int launch_clusters(emsar_hip_ctx *ctx, const SetSolveParams &P, double *theta) {
    const SetsDev &D = ctx->sets;
    const auto &CL = D.RS.CL;
    HIPCHK(hipMemsetAsync(D.d_cbar, 0, (size_t)D.n_cstat * 2 * sizeof(unsigned), ctx->side[2]));
    HIPCHK(hipEventRecord(ctx->ev_c0, ctx->side[2]));
    size_t first = 0;
    while (first < CL.desc.size()) {
        size_t last = first, wgs = 0;
        while (last < CL.desc.size() && (wgs == 0 || wgs + CL.desc[last].g <= (size_t)ctx->n_cu)) wgs += CL.desc[last++].g;
        hipLaunchKernelGGL(k_solve_cluster, dim3((unsigned)wgs), dim3(emsar::kClusterThreads), CL.max_lds, ctx->side[2], D.d_cdesc, D.d_cblk, CL.desc[first].blk0,
                           D.d_cg_tid, D.d_cg_u, D.d_crow_w, D.d_crp, D.d_cent, D.d_ccp, D.d_ccrow, D.d_cpart, D.d_cscratch, D.d_cbar, D.d_cbar + D.n_cstat,
                           ctx->vec.d_den, theta, D.d_cstat, P);
        first = last;
    }
    HIPCHK(hipEventRecord(ctx->ev_c1, ctx->side[2]));
    // The workgroups of a cluster wait for each other inside the launch, so all of them must get a CU: nothing else may hold CUs while
    // the cluster batches run (k_solve_sets<512> asks for most of a CU's LDS too).  The size classes start after the clusters.
    HIPCHK(hipStreamWaitEvent(ctx->side[0], ctx->ev_c1, 0));
    HIPCHK(hipStreamWaitEvent(ctx->side[1], ctx->ev_c1, 0));
    HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->ev_c1, 0));
    return EMSAR_HIP_OK;
}

// closed-form transcripts and every LDS-resident set, written into theta (the streamed sets' entries are left alone)
int solve_resident_sets(emsar_hip_ctx *ctx, const SetSolveParams &P, const SetSolveParams &Pcluster, double *theta) {
    const SetsDev &D = ctx->sets;
    const auto &S = D.RS;
    int rc;
    hipLaunchKernelGGL(k_closed_form, dim3(grid_for(ctx->n_tx, 256)), dim3(256), 0, ctx->stream, ctx->n_tx, D.d_kind, D.d_usum, ctx->vec.d_den, theta);
    const size_t off[3] = {0, S.desc[0].size(), S.desc[0].size() + S.desc[1].size()};      // per-set results in class order
    if ((rc = fork_side_streams(ctx, 3))) return rc;
    if (D.n_cstat > 0 && (rc = launch_clusters(ctx, Pcluster, theta))) return rc;
    return launch_set_classes(ctx, 3, [&](int c, int threads, hipStream_t st) {
        hipLaunchKernelGGL(kSolveSets[c], dim3((unsigned)S.desc[c].size()), dim3(threads),
                           S.max_lds[c], st, D.d_sdesc[c], D.d_g_tid, D.d_g_u, D.d_row_w, D.d_srp, D.d_sent, D.d_scp, D.d_scrow, ctx->vec.d_den, theta,
                           D.d_sstat + off[c], P);
    });
}

// ---- the streaming passes -----------------------------------------------------------------------------------------------------------

// What k_update applies to a pass besides its vectors: the floors of the stopping rule (abs_floor in theta, count_floor in reads),
// emsar_em_params.zero_cut, and the transcripts the rule leaves out (sets.d_kind while the stream runs next to resident sets, else null)
struct PassRules { double abs_floor, count_floor, zero_cut; const uint8_t *delta_mask; };

// th_out = EM(th_in); ll slot receives sum R log S at th_in when want_ll
int em_pass(emsar_hip_ctx *ctx, const PassRules &R, const double *th_in, double *th_out, bool want_ll, int ll_slot, int to_delta1 = 0) {
    int rc = launch_pass(ctx, want_ll ? MODE_EM_LL : MODE_EM, th_in, ctx->vec.d_acc, &ctx->d_scal->ll[ll_slot].s[0].v);
    if (rc) return rc;
    hipLaunchKernelGGL(k_update, dim3(std::min(grid_for(ctx->n_tx, 256), ctx->update_grid)), dim3(256), 0, ctx->stream, ctx->n_tx, th_in, ctx->vec.d_acc,
                       ctx->vec.d_den, ctx->layout == EMSAR_LAYOUT_TILED ? ctx->lay.d_u.get() : nullptr, th_out, R.abs_floor, R.count_floor, R.zero_cut, ctx->d_scal,
                       R.delta_mask, to_delta1, fx_of(ctx).mass);
    HIPCHK(hipGetLastError());
    return EMSAR_HIP_OK;
}

// `cycles` cycles of the streaming solve on ctx->stream -- launched, or recorded when the stream is capturing.
// One cycle = one plain EM pass, or one SQUAREM cycle of three passes (8 launches, see k_update_p2).  The current point is
// ctx->vec.d_th[0] before and after (plain EM swaps d_th[0]/d_th[1] on the host: record an even count).
int enqueue_cycles(emsar_hip_ctx *ctx, const PassRules &R, bool accel, double abs_step_base, int cycles) {
    const int n = ctx->n_tx, g = grid_for(n, 256);
    DevBuf<double> *th = ctx->vec.d_th;     // handles: plain EM swaps two of them
    int rc;
    for (int c = 0; c < cycles; c++) {
        hipLaunchKernelGGL(k_cycle_begin, dim3(1), dim3(kLlSlots), 0, ctx->stream, ctx->d_scal, abs_step_base, accel ? 3 : 1);
        if (!accel) {
            if ((rc = em_pass(ctx, R, th[0], th[1], false, 0))) return rc;
            std::swap(th[0], th[1]);
            continue;
        }
        // the stopping rule is measured on the first (plain) step of the cycle only (delta1_bits)
        const double *u = ctx->layout == EMSAR_LAYOUT_TILED ? ctx->lay.d_u.get() : nullptr;
        const dim3 gv((unsigned)std::min(std::min(g, ctx->sq_grid), kSqPart)), bv(256);
        if ((rc = em_pass(ctx, R, th[0], th[1], false, 0, 1))) return rc;
        if ((rc = launch_pass(ctx, MODE_EM_LL, th[1], ctx->vec.d_acc, &ctx->d_scal->ll[1].s[0].v, true))) return rc;
        hipLaunchKernelGGL(k_update_p2, gv, bv, 0, ctx->stream, n, th[0], th[1], ctx->vec.d_acc, ctx->vec.d_den, u, th[2], ctx->d_scal, ctx->d_sqpart, fx_of(ctx));
        hipLaunchKernelGGL(k_sq_extrap_ll, gv, bv, 0, ctx->stream, n, th[0], th[1], th[2], ctx->vec.d_den, u, th[3], ctx->d_scal, ctx->d_sqpart, (int)gv.x, fx_of(ctx));
        if ((rc = launch_pass(ctx, MODE_EM_LL, th[3], ctx->vec.d_acc, &ctx->d_scal->ll[2].s[0].v, true))) return rc;
        hipLaunchKernelGGL(k_update_p3, gv, bv, 0, ctx->stream, n, th[3], th[2], ctx->vec.d_acc, ctx->vec.d_den, u, th[0], ctx->d_scal, ctx->d_sqpart, (int)gv.x, fx_of(ctx));
        HIPCHK(hipGetLastError());
    }
    return EMSAR_HIP_OK;
}

struct CycleGraph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    ~CycleGraph() {
        if (exec) (void)hipGraphExecDestroy(exec);
        if (graph) (void)hipGraphDestroy(graph);
    }
};

// ---- one solve ------------------------------------------------------------------------------------------------------------------------

// the caller's parameters with the defaults filled in
emsar_em_params solve_params(const emsar_em_params *pp) {
    emsar_em_params p = pp ? *pp : emsar_em_params{0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (p.max_iter <= 0) p.max_iter = 100000;
    if (p.tol <= 0) p.tol = 1e-10;
    if (p.abs_floor <= 0) p.abs_floor = 1e-6;
    if (p.check_every <= 0) p.check_every = 8;
    return p;
}
// what the resident sets get of them
SetSolveParams set_params(const emsar_em_params &p) {
    // zero_cut / abs_step exist because a boundary optimum is approached like 1/k by the EM; the sets that get Newton steps reach it
    // in a few steps and are held to the strict rule (same pass counts with and without the two rules on every problem measured,
    // and then nothing is printed differently); the rules stay in force for the streamed part and with newton_after < 0
    const bool strict_sets = p.newton_after >= 0;
    return SetSolveParams{p.tol, p.abs_floor, p.count_floor, (!strict_sets && p.zero_cut > 0.0) ? p.zero_cut : 0.0,
                          (!strict_sets && p.abs_step > 0.0) ? p.abs_step : 0.0, p.max_iter, p.accel, p.newton_after == 0 ? 60 : p.newton_after};
}

// What a solve runs: the set solver when asked for (set_mode 0; the sets are found on first use) unless one component holds most
// transcripts (giant: plain streaming solve), and the streaming passes when there are no sets or for the sets that fit no workgroup.
struct SolvePlan { bool use_sets = false, need_stream = true; };
int plan_solve(emsar_hip_ctx *ctx, int set_mode, SolvePlan &out) {
    out.use_sets = set_mode == 0;
    if (out.use_sets) { if (const int rc = ensure_sets(ctx)) return rc; }
    if (out.use_sets && ctx->sets.RS.giant) out.use_sets = false;
    out.need_stream = !out.use_sets || ctx->sets.RS.n_streamed_sets > 0;
    return EMSAR_HIP_OK;
}

// One solve from the start point of emsar_hip_reset_theta: parameters, plan, counters, and the stages in the order of run().
// On the context's stream: ev0, cycles, ev1, closed form + resident sets + clusters + their statistics' copies, ev2, the likelihood
// pass, the two copies, one synchronise.
struct SolveRun {
    emsar_hip_ctx *const ctx;
    const emsar_em_params p;             // the caller's parameters with the defaults filled in
    double *const fpkm_out;
    emsar_em_stats *const stats;         // may be null
    const double abs_step_base;
    const int per_cycle;                 // passes of a cycle: 1 plain EM, 3 SQUAREM
    SolvePlan plan;
    PassRules rules{0.0, 0.0, 0.0, nullptr};
    std::chrono::steady_clock::time_point t0;
    int iters = 0, cycles = 0, converged = 0;     // streaming passes and cycles done
    double delta = 0.0;                  // the stopping rule's measure: of the stream at the last poll, then the largest over the sets
    CycleGraph G;                        // check_every cycles, captured at most once
    int64_t graph_launches = 0;
    int32_t set_max = 0, cl_max = 0, set_unconv = 0;   // over the resident sets and the clusters
    int64_t set_sum = 0;

    SolveRun(emsar_hip_ctx *c, const emsar_em_params *pp, double *out, emsar_em_stats *st)
        : ctx(c), p(solve_params(pp)), fpkm_out(out), stats(st), abs_step_base(p.abs_step > 0.0 ? p.abs_step : 0.0), per_cycle(p.accel ? 3 : 1) {}

    // arguments, which solvers run, the rules of a streaming pass, the start point; ev0
    int begin() {
        if (!(p.count_floor >= 0.0)) return EMSAR_HIP_ERR_ARG;
        if (p.set_mode != 0 && p.set_mode != 1) return EMSAR_HIP_ERR_ARG;
        HIPCHK(hipSetDevice(ctx->device));
        int rc;
        if ((rc = plan_solve(ctx, p.set_mode, plan))) return rc;
        // next to resident sets the stream's stopping rule looks at the streamed sets' transcripts only
        rules = PassRules{p.abs_floor, p.count_floor, p.zero_cut > 0.0 ? p.zero_cut : 0.0, plan.use_sets && plan.need_stream ? ctx->sets.d_kind.get() : nullptr};
        converged = plan.need_stream ? 0 : 1;
        delta = plan.need_stream ? INFINITY : 0.0;
        t0 = std::chrono::steady_clock::now();
        if ((rc = emsar_hip_reset_theta(ctx))) return rc;
        hipLaunchKernelGGL(k_scal_init, dim3(1), dim3(1), 0, ctx->stream, ctx->d_scal);
        HIPCHK(hipEventRecord(ctx->ev0, ctx->stream));
        return EMSAR_HIP_OK;
    }
    // check_every cycles from the graph, captured on first use: on the context's one stream, thread-local mode, a single-stream chain
    int replay_cycles() {
        if (!G.exec) {
            HIPCHK(hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
            const int rc = enqueue_cycles(ctx, rules, p.accel != 0, abs_step_base, p.check_every);
            const hipError_t e = hipStreamEndCapture(ctx->stream, &G.graph);      // always closes the capture
            if (rc) return rc;
            HIPCHK(e);
            HIPCHK(hipGraphInstantiate(&G.exec, G.graph, nullptr, nullptr, 0));
        }
        HIPCHK(hipGraphLaunch(G.exec, ctx->stream));
        graph_launches++;
        return EMSAR_HIP_OK;
    }
    // the host's look at the stopping rule: delta of the last cycle (SQUAREM: of its first, plain step)
    int poll() {
        HIPCHK(hipMemcpyAsync(ctx->h_scal, ctx->d_scal, sizeof(Scal), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        const unsigned long long bits = p.accel ? ctx->h_scal->delta1_bits : ctx->h_scal->delta_bits;
        memcpy(&delta, &bits, 8);
        if (!std::isfinite(delta) || ctx->h_scal->bad) { ctx->err = "non-finite theta"; return EMSAR_HIP_ERR_NUMERIC; }
        return EMSAR_HIP_OK;
    }
    // The streaming passes; ev1.  The first 4 x check_every cycles are launched kernel by kernel (a quick solve never pays for a
    // graph); after that check_every cycles are recorded once into a hipGraph and replayed between the host's looks at the stopping
    // rule.  Measured gain: 1-5 % on problems of 40 k .. 2 M rows (tools/graph_bench.py) -- the launches were already asynchronous,
    // and a pass of a small problem costs one workgroup's latency (12-26 us), not its launch.
    int stream() {
        const int ce = p.check_every;
        const bool graph_ok = ctx->use_graph && (p.accel || ce % 2 == 0);   // plain EM swaps th0/th1: an even count restores them
        int rc;
        while (plan.need_stream && iters < p.max_iter) {
            int todo = 1;
            if (graph_ok && cycles >= 4 * ce && cycles % ce == 0 && (int64_t)iters + (int64_t)per_cycle * ce <= (int64_t)p.max_iter) {
                todo = ce;
                if ((rc = replay_cycles())) return rc;
            } else if ((rc = enqueue_cycles(ctx, rules, p.accel != 0, abs_step_base, 1))) return rc;
            cycles += todo;
            iters += todo * per_cycle;
            if (cycles % ce == 0 || iters >= p.max_iter) {
                if ((rc = poll())) return rc;
                if (delta < p.tol) { converged = 1; break; }
            }
        }
        HIPCHK(hipEventRecord(ctx->ev1, ctx->stream));
        return EMSAR_HIP_OK;
    }
    // closed form, resident sets and clusters into the current point, their statistics on the way to the host; ev2
    int resident_sets() {
        if (plan.use_sets) {
            const SetSolveParams P = set_params(p);
            // the cluster solver has no Newton step: its sets keep the two print-quantum rules whatever newton_after says (with the strict rule
            // alone a boundary optimum keeps a cluster going for 10^5 passes at ~32 us each)
            SetSolveParams Pc = P;
            Pc.zero_cut = rules.zero_cut;
            Pc.abs_step = abs_step_base;
            const SetsDev &D = ctx->sets;
            if (const int rc = solve_resident_sets(ctx, P, Pc, ctx->vec.d_th[0])) return rc;
            if (D.n_sstat > 0) HIPCHK(hipMemcpyAsync(D.h_sstat, D.d_sstat, (size_t)D.n_sstat * sizeof(SetStat), hipMemcpyDeviceToHost, ctx->stream));
            if (D.n_cstat > 0) HIPCHK(hipMemcpyAsync(D.h_cstat, D.d_cstat, (size_t)D.n_cstat * sizeof(ClusterStat), hipMemcpyDeviceToHost, ctx->stream));
        }
        HIPCHK(hipEventRecord(ctx->ev2, ctx->stream));
        return EMSAR_HIP_OK;
    }
    // F at the returned point: one likelihood-only pass (not counted in iters); theta to the caller, in the caller's numbering
    int likelihood_and_fetch() {
        const int n = ctx->n_tx;
        double *const th0 = ctx->vec.d_th[0];
        hipLaunchKernelGGL(k_cycle_begin, dim3(1), dim3(kLlSlots), 0, ctx->stream, ctx->d_scal, 0.0, 0);
        if (const int rc = launch_pass(ctx, MODE_EM_LL, th0, ctx->vec.d_acc, &ctx->d_scal->ll[0].s[0].v)) return rc;
        HIPCHK(hipMemsetAsync(ctx->vec.d_acc, 0, (size_t)n * 8, ctx->stream));
        hipLaunchKernelGGL(k_dot, dim3(1), dim3(1024), 0, ctx->stream, n, th0, ctx->vec.d_den, &ctx->d_scal->ll[3].s[0].v);
        HIPCHK(hipMemcpyAsync(ctx->h_scal, ctx->d_scal, sizeof(Scal), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(fpkm_out, th0, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        try { from_lib(ctx, fpkm_out); } catch (const std::bad_alloc &) { return EMSAR_HIP_ERR_OOM; }
        if (getenv("EMSAR_HIP_DEBUG"))
            fprintf(stderr, "emsar_hip_solve: %d streaming passes, %lld graph replays of %d cycles\n", iters, (long long)graph_launches, p.check_every);
        for (int32_t t = 0; t < n; t++)
            if (!std::isfinite(fpkm_out[t])) { ctx->err = "non-finite theta"; return EMSAR_HIP_ERR_NUMERIC; }
        return EMSAR_HIP_OK;
    }
    // the per-set results of one family: the slowest set, the sum of passes, the unconverged, the largest delta
    static bool gave_up(const SetStat &) { return false; }
    static bool gave_up(const ClusterStat &q) { return q.aborted != 0; }
    template <class Stat> int collect(const Stat *h, int64_t count, int32_t &passes_max) {
        for (int64_t i = 0; i < count; i++) {
            const Stat &q = h[i];
            if (gave_up(q)) { ctx->err = "a workgroup cluster gave up waiting at its barrier"; return EMSAR_HIP_ERR_HIP; }
            passes_max = std::max(passes_max, q.passes); set_sum += q.passes;
            if (!q.converged) set_unconv++;
            if (!std::isfinite(q.delta)) { ctx->err = "non-finite theta in a connected set"; return EMSAR_HIP_ERR_NUMERIC; }
            if (q.delta > delta) delta = q.delta;
        }
        return EMSAR_HIP_OK;
    }
    int collect_set_stats() {
        if (!plan.use_sets) return EMSAR_HIP_OK;
        int rc;
        if ((rc = collect(ctx->sets.h_sstat.get(), ctx->sets.n_sstat, set_max)) || (rc = collect(ctx->sets.h_cstat.get(), ctx->sets.n_cstat, cl_max))) return rc;
        set_max = std::max(set_max, cl_max);
        if (set_unconv) converged = 0;
        return EMSAR_HIP_OK;
    }
    int fill_stats() {
        if (!stats) return EMSAR_HIP_OK;
        const auto &S = ctx->sets.RS;
        float ms = 0, ms_sets = 0;
        HIPCHK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        HIPCHK(hipEventElapsedTime(&ms_sets, ctx->ev1, ctx->ev2));
        memset(stats, 0, sizeof(*stats));
        stats->iters = iters + set_max;
        stats->converged = converged;
        stats->final_delta = delta;
        stats->loglik = host_ll(ctx, 0) + ctx->loglik_const - ctx->h_scal->ll[3].s[0].v;
        stats->kernel_ms = ms + (plan.use_sets ? ms_sets : 0.0f);
        stats->solve_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        stats->bytes_per_pass = ctx->bytes_formula;
        stats->stored_bytes_per_pass = stored_bytes(ctx);
        if (p.set_mode == 0 && S.giant) { stats->sets_streamed = 1; stats->sets_build_ms = ctx->sets_build_ms; }
        if (!plan.use_sets) return EMSAR_HIP_OK;
        stats->sets_resident = (int32_t)S.n_resident();
        stats->sets_streamed = (int32_t)S.n_streamed_sets;
        stats->set_passes_max = set_max;
        stats->sets_unconverged = set_unconv;
        stats->set_passes_sum = set_sum;
        stats->sets_build_ms = ctx->sets_build_ms;
        stats->sets_kernel_ms = ms_sets;
        stats->sets_cluster = (int32_t)ctx->sets.n_cstat;
        stats->cluster_passes_max = cl_max;
        if (ctx->sets.n_cstat > 0) { float mc = 0; HIPCHK(hipEventElapsedTime(&mc, ctx->ev_c0, ctx->ev_c1)); stats->cluster_kernel_ms = mc; }
        return EMSAR_HIP_OK;
    }
    int run() {
        int rc;
        if ((rc = begin()) || (rc = stream()) || (rc = resident_sets()) || (rc = likelihood_and_fetch()) || (rc = collect_set_stats())) return rc;
        return fill_stats();
    }
};

}  // namespace

extern "C" {

int emsar_hip_run_passes(emsar_hip_ctx *ctx, int32_t n_passes, float *elapsed_ms, double *last_ll) {
    if (!ctx || n_passes < 0) return EMSAR_HIP_ERR_ARG;
    if (!ctx->have_sample) return EMSAR_HIP_ERR_STATE;
    HIPCHK(hipSetDevice(ctx->device));
    const PassRules rules{1e-6, 0.0, 0.0, nullptr};
    hipLaunchKernelGGL(k_cycle_begin, dim3(1), dim3(kLlSlots), 0, ctx->stream, ctx->d_scal, 0.0, 0);
    HIPCHK(hipEventRecord(ctx->ev0, ctx->stream));
    int cur = 0;  // th[cur] holds the current point, th[cur^1] receives the next
    for (int i = 0; i < n_passes; i++) {
        bool ll = last_ll && i == n_passes - 1;
        int rc = em_pass(ctx, rules, ctx->vec.d_th[cur], ctx->vec.d_th[cur ^ 1], ll, 0);
        if (rc) return rc;
        cur ^= 1;
    }
    HIPCHK(hipEventRecord(ctx->ev1, ctx->stream));
    if (cur == 1) HIPCHK(hipMemcpyAsync(ctx->vec.d_th[0], ctx->vec.d_th[1], (size_t)ctx->n_tx * 8, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->h_scal, ctx->d_scal, sizeof(Scal), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (elapsed_ms) HIPCHK(hipEventElapsedTime(elapsed_ms, ctx->ev0, ctx->ev1));
    if (last_ll) *last_ll = host_ll(ctx, 0);
    return EMSAR_HIP_OK;
}

int emsar_hip_solve(emsar_hip_ctx *ctx, const emsar_em_params *pp, double *fpkm_out, emsar_em_stats *stats) {
    if (!ctx || !fpkm_out) return EMSAR_HIP_ERR_ARG;
    if (!ctx->have_sample) return EMSAR_HIP_ERR_STATE;
    return SolveRun(ctx, pp, fpkm_out, stats).run();
}

}  // extern "C"
