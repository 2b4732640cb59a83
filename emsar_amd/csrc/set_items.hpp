// set_items.hpp -- what the drivers of the resident sets share beyond solve.hpp: the batch rule (item_batch), the item runner of a
// set-kernel family whose workgroups each take one item and leave one record (SetItemRunner: presence.hpp, profile.hpp, compare.hpp),
// the locator of a call's queried transcripts (SetQuery), what the two-sample and gene-level drivers ask of a context (side_of,
// launch_class_lds, add_search_stats) and the frames of the calls (query_ok, gene_query_ok, two_samples_ok, run_query_call,
// run_two_sample_call).  Part of emsar_hip.hip's translation unit, included after solve.hpp.

namespace {

inline size_t free_device_bytes() { size_t f = 0, t = 0; return hipMemGetInfo(&f, &t) == hipSuccess ? f : (size_t)1 << 30; }

// Units of work per batch: what fits a quarter of the free device memory (at most 2 GiB) at per_item_bytes each; the environment
// variable env_name overrides it (a value >= 1); never more than there are (most) nor than a launch takes (cap)
inline int64_t item_batch(int64_t per_item_bytes, const char *env_name, int64_t most, int64_t cap) {
    const int64_t budget = std::min<int64_t>((int64_t)(free_device_bytes() / 4), (int64_t)2 << 30);
    int64_t batch = std::max<int64_t>(1, budget / per_item_bytes);
    if (const char *env = getenv(env_name)) { if (atoi(env) >= 1) batch = atoi(env); }
    return std::min<int64_t>(std::min<int64_t>(batch, most), cap);
}

// the descriptor of set `set` of size class c of the context, null where there is none: the bounds check of an item's set
inline const emsar::SetDesc *set_desc(const emsar_hip_ctx *ctx, int c, int32_t set) {
    if (c < 0 || c >= emsar::kSetClasses || set < 0 || (size_t)set >= ctx->sets.RS.desc[c].size()) return nullptr;
    return &ctx->sets.RS.desc[c][(size_t)set];
}
// the set records of the context's sample, as the two-sample and the gene-level kernels take them
inline CompareSide side_of(const emsar_hip_ctx *c) {
    const SetsDev &D = c->sets;
    return CompareSide{D.d_sdesc[0].get(), D.d_sdesc[1].get(), D.d_sdesc[2].get(), D.d_g_tid.get(), D.d_g_u.get(), D.d_row_w.get(),
                       D.d_srp.get(), D.d_sent.get(), D.d_scp.get(), D.d_scrow.get(), c->vec.d_den.get()};
}
// The LDS of a launch class whose items may hold sets of their own class and of every smaller one, of context a and (when given) b
inline void launch_class_lds(size_t (&lds)[emsar::kSetClasses], const emsar_hip_ctx *a, const emsar_hip_ctx *b = nullptr) {
    size_t most = 0;
    for (int c = 0; c < emsar::kSetClasses; c++) {
        most = std::max(most, (size_t)a->sets.RS.max_lds[c]);
        if (b) most = std::max(most, (size_t)b->sets.RS.max_lds[c]);
        lds[c] = most;
    }
}
// a search record into the statistics of its call
template <class Stats, class Rec>
inline void add_search_stats(Stats &st, const Rec &r) {
    st.evals_sum += r.evals; st.passes_sum += r.passes;
    st.evals_max = std::max(st.evals_max, r.evals); st.passes_max = std::max(st.passes_max, r.passes);
}

// Items of the three launch classes through one family of set kernels, at most a batch per class and launch, the classes next to each
// other on the streams of `ctx`; recs[c][i] answers items[c][i].
template <class Item, class Rec>
struct SetItemRunner {
    emsar_hip_ctx *const ctx;
    const char *batch_env;               // the variable that overrides the batch; the owner of a borrowed run may name its own
    const char *const bad_item;          // ctx->err of an item that fails the check
    DevBuf<Item> d_items[emsar::kSetClasses];
    DevBuf<Rec> d_rec[emsar::kSetClasses];
    hipEvent_t e[2] = {nullptr, nullptr};

    SetItemRunner(emsar_hip_ctx *c, const char *env, const char *bad) : ctx(c), batch_env(env), bad_item(bad) {}
    ~SetItemRunner() { for (hipEvent_t ev : e) if (ev) (void)hipEventDestroy(ev); }

    // valid(class, item): the family's whole check -- the item's sets against their descriptors (set_desc) and its own fields --, made on
    // every item before anything is launched;
    // launch(class, threads, stream, count, d_items, d_rec): the family's kernel on `count` items, its LDS attributes set by the caller.
    // A class is launched when it has items, the big classes first (launch_set_classes' order, which asks for sets in the class of `ctx`
    // instead: an item of the compare family may run in a class in which ctx has none).  The device time of the launches is added to
    // ms_acc, the items to `launched`.
    template <class Valid, class Launch>
    int run(const std::vector<Item> (&items)[emsar::kSetClasses], std::vector<Rec> (&recs)[emsar::kSetClasses], double &ms_acc, int64_t &launched,
            const Valid &valid, const Launch &launch) {
        size_t most = 0;
        for (int c = 0; c < emsar::kSetClasses; c++) {
            for (const Item &it : items[c]) if (!valid(c, it)) { ctx->err = bad_item; return EMSAR_HIP_ERR_HIP; }
            recs[c].resize(items[c].size());
            most = std::max(most, items[c].size());
        }
        if (most == 0) return EMSAR_HIP_OK;
        const size_t batch = (size_t)item_batch((int64_t)(emsar::kSetClasses * (sizeof(Item) + sizeof(Rec))), batch_env, (int64_t)most, (int64_t)1 << 20);
        for (int c = 0; c < emsar::kSetClasses; c++)
            if (!items[c].empty()) {
                const size_t cnt = std::min(batch, items[c].size());
                HIPCHK(d_items[c].alloc(cnt)); HIPCHK(d_rec[c].alloc(cnt));
            }
        for (hipEvent_t &ev : e) if (!ev) HIPCHK(hipEventCreate(&ev));
        const hipStream_t st[emsar::kSetClasses] = {ctx->stream, ctx->side[0], ctx->side[1]};
        for (size_t first = 0; first < most; first += batch) {
            size_t cnt[emsar::kSetClasses];
            for (int c = 0; c < emsar::kSetClasses; c++) {
                cnt[c] = items[c].size() > first ? std::min(batch, items[c].size() - first) : 0;
                if (cnt[c]) HIPCHK(hipMemcpyAsync(d_items[c], items[c].data() + first, cnt[c] * sizeof(Item), hipMemcpyHostToDevice, ctx->stream));
            }
            HIPCHK(hipEventRecord(e[0], ctx->stream));
            if (const int rc = fork_side_streams(ctx, 2)) return rc;
            for (int c = emsar::kSetClasses - 1; c >= 0; c--) if (cnt[c]) launch(c, emsar::kSetThreads[c], st[c], cnt[c], d_items[c].get(), d_rec[c].get());
            for (int i = 0; i < 2; i++) {
                HIPCHK(hipEventRecord(ctx->ev_join[i], ctx->side[i]));
                HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->ev_join[i], 0));
            }
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(e[1], ctx->stream));
            for (int c = 0; c < emsar::kSetClasses; c++)
                if (cnt[c]) HIPCHK(hipMemcpyAsync(recs[c].data() + first, d_rec[c], cnt[c] * sizeof(Rec), hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipStreamSynchronize(ctx->stream));
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, e[0], e[1]));
            ms_acc += ms;
            for (int c = 0; c < emsar::kSetClasses; c++) launched += (int64_t)cnt[c];
        }
        return EMSAR_HIP_OK;
    }
};

// Where the queried transcripts of a per-transcript call stand in one context before anything is solved: what the presence test, the
// profile intervals (through it) and the two-sample test (once per sample) need to know first.  plan, then classify.
struct SetQuery {
    enum Standing : int32_t {
        OUTSIDE,                         // den is not > 0: outside the likelihood
        NOT_RESIDENT,                    // in a streamed set or a cluster, or the solve would not use the sets at all
        CLOSED,                          // a one-transcript component: `u` reads on the transcript alone
        MEMBER                           // transcript `loc` of packed set `set` of size class `cls`
    };
    // one queried transcript (library index), once however often it is asked for
    struct Cand {
        int32_t lib, cls = -1, set = -1, loc = -1;
        int32_t standing = NOT_RESIDENT;
        bool own_reads = false;          // MEMBER: a single-transcript row of its own has reads
        double u = 0.0;                  // CLOSED: its read count
    };
    emsar_hip_ctx *const ctx;
    const emsar_em_params p;             // the caller's parameters with the defaults filled in
    const int32_t nq;
    const int32_t *const query;          // caller tids, null = all in order
    const int n;
    bool use_sets = false;
    std::vector<Cand> cand;
    std::vector<int32_t> cand_of_lib;    // [n] -> cand, -1 = not queried
    std::vector<double> h_den, h_usum, h_gu;       // [n] [n] [resident tids]: den, closed-form counts, folded counts (use_sets only)
    std::vector<int32_t> h_gtid;                   // [resident tids]

    SetQuery(emsar_hip_ctx *c, const emsar_em_params *pp, int32_t nq_, const int32_t *q) : ctx(c), p(solve_params(pp)), nq(nq_), query(q), n(c->n_tx) {}

    int32_t lib_of(int32_t tid) const { return renumbered(ctx) ? tid_map(ctx)[(size_t)tid] : tid; }
    // the candidate of the i-th query
    size_t cand_index(int32_t i) const { return (size_t)cand_of_lib[(size_t)lib_of(query ? query[i] : i)]; }

    // which solvers a solve would run (the sets are found on first use: ensure_sets), and the query with its repeats removed
    int plan() {
        if (!(p.count_floor >= 0.0) || (p.set_mode != 0 && p.set_mode != 1)) return EMSAR_HIP_ERR_ARG;
        SolvePlan sp;
        if (const int rc = plan_solve(ctx, p.set_mode, sp)) return rc;
        use_sets = sp.use_sets;
        cand_of_lib.assign((size_t)n, -1);
        for (int32_t i = 0; i < nq; i++) {
            const int32_t l = lib_of(query ? query[i] : i);
            if (cand_of_lib[(size_t)l] >= 0) continue;
            cand_of_lib[(size_t)l] = (int32_t)cand.size();
            Cand c; c.lib = l;
            cand.push_back(c);
        }
        return EMSAR_HIP_OK;
    }

    // The packed sets' transcript lists and folded counts live on the device only (ensure_sets frees the host copies): they are read
    // back here, with den and the closed-form counts.
    int classify() {
        if (!use_sets) return EMSAR_HIP_OK;          // every candidate NOT_RESIDENT
        const SetsDev &D = ctx->sets;
        const auto &S = D.RS;
        size_t n_gu = 0;
        for (int c = 0; c < emsar::kSetClasses; c++) for (const auto &d : S.desc[c]) n_gu = std::max<size_t>(n_gu, (size_t)d.tid_off + d.n_t);
        h_den.resize((size_t)n); h_usum.resize((size_t)n); h_gtid.resize(n_gu); h_gu.resize(n_gu);
        if (n > 0) {
            HIPCHK(hipMemcpyAsync(h_den.data(), ctx->vec.d_den, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipMemcpyAsync(h_usum.data(), D.d_usum, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
        }
        if (n_gu > 0) {
            HIPCHK(hipMemcpyAsync(h_gtid.data(), D.d_g_tid, n_gu * 4, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipMemcpyAsync(h_gu.data(), D.d_g_u, n_gu * 8, hipMemcpyDeviceToHost, ctx->stream));
        }
        HIPCHK(hipStreamSynchronize(ctx->stream));
        for (int c = 0; c < emsar::kSetClasses; c++)
            for (size_t s = 0; s < S.desc[c].size(); s++) {
                const emsar::SetDesc &d = S.desc[c][s];
                for (uint32_t i = 0; i < d.n_t; i++) {
                    const int32_t k = cand_of_lib[(size_t)h_gtid[d.tid_off + i]];
                    if (k >= 0) { cand[(size_t)k].cls = c; cand[(size_t)k].set = (int32_t)s; cand[(size_t)k].loc = (int32_t)i; }
                }
            }
        for (auto &c : cand) {
            const uint8_t kind = S.kind[(size_t)c.lib];
            if (!(h_den[(size_t)c.lib] > 0.0)) c.standing = OUTSIDE;
            else if (kind == emsar::KIND_STREAMED || kind == emsar::KIND_CLUSTER) c.standing = NOT_RESIDENT;
            else if (kind == emsar::KIND_CLOSED) { c.standing = CLOSED; c.u = h_usum[(size_t)c.lib]; }
            else if (c.set < 0) { ctx->err = "presence: a resident transcript is in no packed set"; return EMSAR_HIP_ERR_HIP; }
            else { c.standing = MEMBER; c.own_reads = h_gu[S.desc[c.cls][(size_t)c.set].tid_off + (size_t)c.loc] > 0.0; }
        }
        return EMSAR_HIP_OK;
    }
};

// The query of a per-transcript call: null = every transcript in order (n_query is set to their number), else n_query tids of the sample
inline int query_ok(const emsar_hip_ctx *ctx, int32_t &n_query, const int32_t *query_tids) {
    if (!ctx) return EMSAR_HIP_ERR_ARG;
    if (!ctx->have_sample) return EMSAR_HIP_ERR_STATE;
    if (!query_tids) n_query = ctx->n_tx;
    if (n_query < 0) return EMSAR_HIP_ERR_ARG;
    if (query_tids) for (int32_t i = 0; i < n_query; i++) if (query_tids[i] < 0 || query_tids[i] >= ctx->n_tx) return EMSAR_HIP_ERR_ARG;
    return EMSAR_HIP_OK;
}
// The query of a per-gene call of a context that holds a gene map: null = every gene in order, else n_query gene ids
inline int gene_query_ok(const emsar_hip_ctx *ctx, int32_t &n_query, const int32_t *query_genes) {
    if (!query_genes) n_query = ctx->genes.n_genes;
    if (n_query < 0) return EMSAR_HIP_ERR_ARG;
    if (query_genes) for (int32_t i = 0; i < n_query; i++) if (query_genes[i] < 0 || query_genes[i] >= ctx->genes.n_genes) return EMSAR_HIP_ERR_ARG;
    return EMSAR_HIP_OK;
}
// the two contexts hold one structure: compared on what they keep on the host
inline bool same_structure(const emsar_hip_ctx *a, const emsar_hip_ctx *b) {
    return a->n_rows == b->n_rows && a->n_tx == b->n_tx && a->nnz == b->nnz && a->h_row_ptr == b->h_row_ptr && a->h_col == b->h_col;
}
// The two contexts of a two-sample call: distinct, each with a sample (a state error whatever the other arguments say), on one device,
// of one structure; genes: ctx_a holds the gene map, and ctx_b's, if it has one, is the same
inline int two_samples_ok(const emsar_hip_ctx *ctx_a, const emsar_hip_ctx *ctx_b, bool genes) {
    if (!ctx_a || !ctx_b || ctx_a == ctx_b) return EMSAR_HIP_ERR_ARG;
    if (!ctx_a->have_sample || !ctx_b->have_sample) return EMSAR_HIP_ERR_STATE;
    if (ctx_a->device != ctx_b->device || !same_structure(ctx_a, ctx_b)) return EMSAR_HIP_ERR_ARG;
    if (!genes) return EMSAR_HIP_OK;
    if (!ctx_a->genes.have_genes) return EMSAR_HIP_ERR_STATE;
    const GeneMap &ga = ctx_a->genes, &gb = ctx_b->genes;
    if (gb.have_genes && (gb.n_genes != ga.n_genes || gb.h_gene_of_tx != ga.h_gene_of_tx)) return EMSAR_HIP_ERR_ARG;
    return EMSAR_HIP_OK;
}
// The frame of a call: the device, the stream drained, one Run(ctx, args...) built and run, total_ms taken, its statistics copied out
template <class Run, class Stats, class... Args>
int run_query_call(emsar_hip_ctx *ctx, Stats *stats, const Args &...args) {
    const auto t0 = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    try {
        Run run(ctx, args...);
        if (const int rc = run.run()) return rc;
        run.st.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = run.st;
    } catch (const std::bad_alloc &) { return EMSAR_HIP_ERR_OOM; }
    return EMSAR_HIP_OK;
}
// The frame of a two-sample call, its arguments checked: ctx_b's stream drained (the launches run on ctx_a's streams), then ctx_a's
// frame with one Run(ctx_a, ctx_b, args...)
template <class Run, class Stats, class... Args>
int run_two_sample_call(emsar_hip_ctx *ctx_a, emsar_hip_ctx *ctx_b, Stats *stats, const Args &...args) {
    emsar_hip_ctx *const ctx = ctx_b;
    HIPCHK(hipSetDevice(ctx_b->device));
    HIPCHK(hipStreamSynchronize(ctx_b->stream));
    return run_query_call<Run>(ctx_a, stats, ctx_b, args...);
}

}  // namespace
