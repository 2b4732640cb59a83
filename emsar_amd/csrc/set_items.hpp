// set_items.hpp -- what the drivers of the resident sets share beyond solve.hpp: the batch rule (item_batch), the item runner of a
// set-kernel family whose workgroups each take one item and leave one record (SetItemRunner: presence.hpp, profile.hpp), and the
// frame of a per-transcript call (query_ok, run_query_call).  Part of emsar_hip.hip's translation unit, included after solve.hpp.

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

// Items of the three size classes through one family of set kernels, at most a batch per class and launch, the classes next to each
// other on their streams; recs[c][i] answers items[c][i].  An Item names its set of the class in `set`.
template <class Item, class Rec>
struct SetItemRunner {
    emsar_hip_ctx *const ctx;
    const char *const batch_env;         // the variable that overrides the batch
    const char *const bad_item;          // ctx->err of an item that fails the check
    DevBuf<Item> d_items[emsar::kSetClasses];
    DevBuf<Rec> d_rec[emsar::kSetClasses];
    hipEvent_t e[2] = {nullptr, nullptr};

    SetItemRunner(emsar_hip_ctx *c, const char *env, const char *bad) : ctx(c), batch_env(env), bad_item(bad) {}
    ~SetItemRunner() { for (hipEvent_t ev : e) if (ev) (void)hipEventDestroy(ev); }

    // valid(item, descriptor of its set): the family's check, made on every item before anything is launched;
    // launch(class, threads, stream, count, d_items, d_rec): the family's kernel on `count` items, its LDS attributes set by the caller.
    // The device time of the launches is added to ms_acc, the items to `launched`.
    template <class Valid, class Launch>
    int run(const std::vector<Item> (&items)[emsar::kSetClasses], std::vector<Rec> (&recs)[emsar::kSetClasses], double &ms_acc, int64_t &launched,
            const Valid &valid, const Launch &launch) {
        const auto &S = ctx->sets.RS;
        size_t most = 0;
        for (int c = 0; c < emsar::kSetClasses; c++) {
            for (const Item &it : items[c])
                if (it.set < 0 || (size_t)it.set >= S.desc[c].size() || !valid(it, S.desc[c][(size_t)it.set])) { ctx->err = bad_item; return EMSAR_HIP_ERR_HIP; }
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
        for (size_t first = 0; first < most; first += batch) {
            int rc;
            size_t cnt[emsar::kSetClasses];
            for (int c = 0; c < emsar::kSetClasses; c++) {
                cnt[c] = items[c].size() > first ? std::min(batch, items[c].size() - first) : 0;
                if (cnt[c]) HIPCHK(hipMemcpyAsync(d_items[c], items[c].data() + first, cnt[c] * sizeof(Item), hipMemcpyHostToDevice, ctx->stream));
            }
            HIPCHK(hipEventRecord(e[0], ctx->stream));
            if ((rc = fork_side_streams(ctx, 2))) return rc;
            rc = launch_set_classes(ctx, 2, [&](int c, int threads, hipStream_t s) { if (cnt[c]) launch(c, threads, s, cnt[c], d_items[c].get(), d_rec[c].get()); });
            if (rc) return rc;
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

// The query of a per-transcript call: null = every transcript in order (n_query is set to their number), else n_query tids of the sample
inline int query_ok(const emsar_hip_ctx *ctx, int32_t &n_query, const int32_t *query_tids) {
    if (!ctx) return EMSAR_HIP_ERR_ARG;
    if (!ctx->have_sample) return EMSAR_HIP_ERR_STATE;
    if (!query_tids) n_query = ctx->n_tx;
    if (n_query < 0) return EMSAR_HIP_ERR_ARG;
    if (query_tids) for (int32_t i = 0; i < n_query; i++) if (query_tids[i] < 0 || query_tids[i] >= ctx->n_tx) return EMSAR_HIP_ERR_ARG;
    return EMSAR_HIP_OK;
}
// Its frame: the device, the stream drained, one Run(ctx, args...) built and run, total_ms taken, its statistics copied out
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

}  // namespace
