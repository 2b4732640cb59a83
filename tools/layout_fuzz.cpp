// Randomised host-side check of the layout builders, meant to be compiled with -fsanitize=address,undefined
// (tests/test_layout_fuzz.py): ragged rows, empty rows, repeated tids, rows too long for a tile, merge on/off.
//   layout_fuzz [N [M]]   N random matrices through build_tiled / check_tiled, M through build_sets / check_sets
//   layout_fuzz digest    one line per case of a fixed corpus (matrix, merge, knobs): name, return code of build_tiled and a
//                         64-bit FNV-1a digest of everything it produced (tests/golden/layout_digests.txt)
#include "../emsar_amd/csrc/layout_tiled.hpp"
#include "../emsar_amd/csrc/sets.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
static bool same_layout(const emsar::TiledLayout &a, const emsar::TiledLayout &b) {
    return a.tiles.size() == b.tiles.size() && (a.tiles.empty() || memcmp(a.tiles.data(), b.tiles.data(), a.tiles.size() * sizeof(emsar::Tile)) == 0) &&
           a.single_row == b.single_row && a.single_tid == b.single_tid && a.slot_row == b.slot_row && a.fwd == b.fwd && a.bwd == b.bwd &&
           a.coo == b.coo && a.far_tid == b.far_tid && a.left_ptr == b.left_ptr && a.left_col == b.left_col && a.left_row == b.left_row &&
           a.mem_ptr == b.mem_ptr && a.mem_row == b.mem_row;
}
struct Matrix { int n_tx = 1, n_rows = 0; std::vector<uint64_t> rp = std::vector<uint64_t>(1, 0); std::vector<int32_t> ci; };
// the matrix of one trial of the fuzz loop: half singletons, a few rows too long for a tile, runs of tids with strays
static Matrix random_matrix(std::mt19937 &rng) {
    Matrix M;
    M.n_tx = 50 + rng() % 5000;
    M.n_rows = rng() % 20000;
    for (int r = 0; r < M.n_rows; r++) {
        int k = rng() % 100 < 50 ? 1 : (rng() % 100 < 2 ? 700 + rng() % 600 : 1 + rng() % 40);
        if (rng() % 50 == 0) k = 0;
        int t0 = rng() % M.n_tx;
        for (int j = 0; j < k; j++) M.ci.push_back(rng() % 10 == 0 ? (int)(rng() % M.n_tx) : std::min(M.n_tx - 1, t0 + j % 64));
        M.rp.push_back(M.ci.size());
    }
    return M;
}

// ---- digest mode ----
struct Fnv {
    uint64_t h = 1469598103934665603ull;
    void bytes(const void *p, size_t n) { const unsigned char *b = (const unsigned char *)p; for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; } }
    template <class T> void val(T v) { bytes(&v, sizeof v); }
    template <class V> void vec(const V &v) { val((uint64_t)v.size()); if (!v.empty()) bytes(v.data(), v.size() * sizeof(v[0])); }
};
static uint64_t layout_digest(const emsar::TiledLayout &L) {
    Fnv f;
    f.vec(L.tiles); f.vec(L.unit_first); f.vec(L.single_row); f.vec(L.single_tid); f.vec(L.slot_row); f.vec(L.fwd); f.vec(L.bwd); f.vec(L.coo);
    f.vec(L.far_tid); f.vec(L.left_ptr); f.vec(L.left_col); f.vec(L.left_row); f.vec(L.mem_ptr); f.vec(L.mem_row); f.vec(L.new_of_old);
    f.val((uint8_t)L.merged); f.val(L.n_rows); f.val(L.n_tx); f.val(L.nnz);
    f.val(L.tiled_entries); f.val(L.far_entries); f.val(L.coo_entries); f.val(L.n_fslices); f.val(L.padded_slots); f.val(L.tiled_ids);
    emsar::UnitTables U;
    emsar::build_unit_tables(L, U);
    f.val((int32_t)U.stride); f.vec(U.utiles);
    return f.h;
}
// rows of `len0 + rng() % len_var` tids: `fam` of them drawn from the row's family of fam_size consecutive tids (0: a run of
// consecutive tids from a random start), the others uniform over all transcripts
static Matrix family_matrix(unsigned seed, int n_tx, int n_rows, int fam_size, int fam, int len0, int len_var) {
    std::mt19937 rng(seed);
    Matrix M;
    M.n_tx = n_tx; M.n_rows = n_rows;
    for (int r = 0; r < n_rows; r++) {
        const int k = len0 + (int)(rng() % len_var), t0 = (int)(rng() % n_tx);
        for (int j = 0; j < k; j++) {
            if (fam_size == 0) M.ci.push_back(std::min(n_tx - 1, t0 + j));
            else if (j < fam) M.ci.push_back(std::min(n_tx - 1, t0 / fam_size * fam_size + (int)(rng() % fam_size)));
            else M.ci.push_back((int)(rng() % n_tx));
        }
        M.rp.push_back(M.ci.size());
    }
    return M;
}
// internal repeats, and rows of exactly kMaxRowLen (the longest a tile takes) and kMaxRowLen + 1 tids (the shortest leftover)
static Matrix repeats_matrix(unsigned seed) {
    std::mt19937 rng(seed);
    Matrix M;
    M.n_tx = 3000; M.n_rows = 4000;
    for (int r = 0; r < M.n_rows; r++) {
        const int k = r % 400 == 7 ? emsar::kMaxRowLen : r % 400 == 9 ? emsar::kMaxRowLen + 1 : 2 + (int)(rng() % 12);
        const int t0 = (int)(rng() % (M.n_tx - k));
        for (int j = 0; j < k; j++) M.ci.push_back(k < 20 && rng() % 4 == 0 && j ? M.ci.back() : t0 + j);
        M.rp.push_back(M.ci.size());
    }
    return M;
}
// the same matrix under a random numbering of the transcripts: the renumbering decided by the sample (EMSAR_HIP_RENUMBER unset) applies
static Matrix shuffled(Matrix M, unsigned seed) {
    std::mt19937 rng(seed);
    std::vector<int32_t> p((size_t)M.n_tx);
    for (int i = 0; i < M.n_tx; i++) p[(size_t)i] = i;
    for (int i = M.n_tx - 1; i > 0; i--) std::swap(p[(size_t)i], p[rng() % (unsigned)(i + 1)]);
    for (int32_t &t : M.ci) t = p[(size_t)t];
    return M;
}
// n_wide rows of wide_len tids anywhere in [0, t0) -- single-tile units closed by the dictionary -- and n_pairs rows (t, t + 1) with t
// anywhere in [t0, t1): units of several tiles, light (one entry per row) or up to the row cap according to the rows per tid.
// One pair row in far_every (0: none) also hits a transcript anywhere in [t1, n_tx): the far list of a unit grows with its rows.
static Matrix pairs_matrix(unsigned seed, int n_wide, int wide_len, int t0, int n_pairs, int t1, int far_every, int n_tx) {
    std::mt19937 rng(seed);
    Matrix M;
    M.n_tx = n_tx; M.n_rows = n_wide + n_pairs;
    for (int r = 0; r < n_wide; r++) {
        for (int j = 0; j < wide_len; j++) M.ci.push_back((int)(rng() % (unsigned)t0));
        M.rp.push_back(M.ci.size());
    }
    for (int r = 0; r < n_pairs; r++) {
        const int t = t0 + (int)(rng() % (unsigned)(t1 - t0 - 1));
        M.ci.push_back(t); M.ci.push_back(t + 1);
        if (far_every && rng() % (unsigned)far_every == 0) M.ci.push_back(t1 + (int)(rng() % (unsigned)(n_tx - t1)));
        M.rp.push_back(M.ci.size());
    }
    return M;
}
struct KnobSet { const char *name; std::vector<std::pair<const char *, const char *>> env; };
static int digest_mode() {
    static const char *const all_knobs[] = {"EMSAR_HIP_TILE_ANCHOR", "EMSAR_HIP_TILE_BLOCK", "EMSAR_HIP_SHORT_ECNT", "EMSAR_HIP_SHORT_BLOCK", "EMSAR_HIP_UNIT_TILES",
        "EMSAR_HIP_TILE_ROWS", "EMSAR_HIP_UNIT_TILES_MAX", "EMSAR_HIP_UNIT_FAR_SOFT", "EMSAR_HIP_TILE_DENSE", "EMSAR_HIP_UNIT_SORT", "EMSAR_HIP_UNIT_LPT",
        "EMSAR_HIP_TILE_CUT", "EMSAR_HIP_FRAG_ROWS", "EMSAR_HIP_TAIL_SPLIT", "EMSAR_HOST_THREADS", "EMSAR_HIP_DEBUG", "EMSAR_HIP_RENUMBER", "EMSAR_HIP_RENUMBER_PAIRS"};
    const std::vector<KnobSet> knobs = {
        {"defaults", {}},
        {"unit_tiles=1", {{"EMSAR_HIP_UNIT_TILES", "1"}}},
        {"unit_tiles=4,max=4", {{"EMSAR_HIP_UNIT_TILES", "4"}, {"EMSAR_HIP_UNIT_TILES_MAX", "4"}}},
        {"tile_rows=768", {{"EMSAR_HIP_TILE_ROWS", "768"}}},
        {"tile_block=128", {{"EMSAR_HIP_TILE_BLOCK", "128"}}},
        {"short_ecnt=3", {{"EMSAR_HIP_SHORT_ECNT", "3"}}},
        {"unit_sort=0", {{"EMSAR_HIP_UNIT_SORT", "0"}}},
        {"unit_lpt=0", {{"EMSAR_HIP_UNIT_LPT", "0"}}},
        {"tile_cut=0", {{"EMSAR_HIP_TILE_CUT", "0"}}},
        {"tile_anchor=0", {{"EMSAR_HIP_TILE_ANCHOR", "0"}}},
        {"far_soft=40", {{"EMSAR_HIP_UNIT_FAR_SOFT", "40"}}},
        {"tail_split=50", {{"EMSAR_HIP_TAIL_SPLIT", "50"}}},
        {"tile_dense=2", {{"EMSAR_HIP_TILE_DENSE", "2"}}},            // refused by the extent check; the arrays are digested all the same
        {"renumber=2", {{"EMSAR_HIP_RENUMBER", "2"}}},
        {"renumber=0", {{"EMSAR_HIP_RENUMBER", "0"}}},
        {"frag_rows=3072,threads=5", {{"EMSAR_HIP_FRAG_ROWS", "3072"}, {"EMSAR_HOST_THREADS", "5"}}},
    };
    auto run = [&](const char *mname, const Matrix &M, int merge, const KnobSet &K) {
        for (const char *k : all_knobs) unsetenv(k);
        for (const auto &kv : K.env) setenv(kv.first, kv.second, 1);
        emsar::TiledLayout L;
        const int rc = emsar::build_tiled(M.n_rows, M.n_tx, M.rp.data(), M.ci.data(), L, merge != 0);
        printf("%s/merge=%d/%s rc=%d %016llx\n", mname, merge, K.name, rc, (unsigned long long)layout_digest(L));
        for (const auto &kv : K.env) unsetenv(kv.first);
    };
    {   // the first matrices of the fuzz loop, merge off and on
        std::mt19937 rng(1);
        for (int trial = 0; trial < 10; trial++) {
            const Matrix M = random_matrix(rng);
            char name[32];
            snprintf(name, sizeof name, "random%d", trial);
            for (int merge = 0; merge < 2; merge++) run(name, M, merge, knobs[0]);
            if (trial == 3 || trial == 6) for (size_t q = 1; q < knobs.size(); q++) run(name, M, (int)(q & 1), knobs[q]);
        }
    }
    // every knob setting on the matrices that take the builder's other branches
    const std::pair<const char *, Matrix> corpus[] = {
        {"runs20", family_matrix(11, 1500, 30000, 0, 0, 16, 9)},              // ~20 consecutive tids: units beyond unit_tiles tiles, too_far / base_rows
        {"runs40", family_matrix(12, 600, 12000, 0, 0, 30, 20)},             // long runs: units closed by the entry cap
        {"family3+far", family_matrix(13, 60000, 40000, 6, 3, 4, 2)},        // 3 in-family tids and 1-2 anywhere: far lists fill, rows are handed back
        {"wide8", family_matrix(14, 40000, 170000, 1, 0, 8, 1)},              // 8 tids anywhere: > 2048 units closed by the dictionary
        {"wide6", family_matrix(15, 25000, 190000, 1, 0, 5, 3)},
        {"repeats", repeats_matrix(16)},
        {"small", family_matrix(17, 900, 500, 8, 3, 3, 3)},                   // one partial slice
        {"empty", Matrix()},
    };
    for (const auto &c : corpus)
        for (size_t q = 0; q < knobs.size(); q++) {
            run(c.first, c.second, 0, knobs[q]);
            if (q == 0 || c.second.n_rows <= 60000) run(c.first, c.second, 1, knobs[q]);
        }
    // matrices made for the knobs that the ones above do not move, each with the defaults and those knobs (merge off: their rows repeat)
    struct Target { const char *name; Matrix M; std::vector<const char *> knobs; };
    const Target targets[] = {
        // 3 in-family tids of 6 under a random numbering: the renumbering applies by default, so renumber=0 differs from it
        {"shuffled6", shuffled(family_matrix(18, 6000, 30000, 6, 3, 3, 2), 19), {"renumber=0"}},
        {"shuffled10", shuffled(family_matrix(20, 9000, 25000, 10, 4, 4, 3), 21), {"renumber=0"}},
        // ~60 rows per tid: units reach the row cap with 40 .. 160 far tids, the range in which UNIT_FAR_SOFT=40 decides too_far
        {"pairs+far80", pairs_matrix(22, 0, 0, 1, 184000, 3000, 80, 200000), {"far_soft=40"}},
        {"pairs+far120", pairs_matrix(23, 0, 0, 1, 200000, 2400, 120, 150000), {"far_soft=40"}},
        // > 2048 units whose lightest are pair units of two tiles: TAIL_SPLIT=50 cuts those into their tiles
        {"wide30+pairs", pairs_matrix(24, 56000, 30, 40000, 700000, 110000, 0, 110000), {"tail_split=50"}},
        {"wide24+pairs", pairs_matrix(25, 70000, 24, 50000, 500000, 100000, 0, 100000), {"tail_split=50"}},
        // runs of 60 .. 80 tids: the entry cap closes a unit in the middle of a slice, and its dictionary fits as it is
        {"runs70", family_matrix(26, 400, 15000, 0, 0, 60, 21), {"tile_cut=0"}},
    };
    for (const Target &t : targets) {
        run(t.name, t.M, 0, knobs[0]);
        for (const char *kn : t.knobs)
            for (const KnobSet &K : knobs) if (!strcmp(K.name, kn)) run(t.name, t.M, 0, K);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "digest")) return digest_mode();
    std::mt19937 rng(1);
    const int n_layout = argc > 1 ? atoi(argv[1]) : 40, n_sets = argc > 2 ? atoi(argv[2]) : 60;
    for (int trial = 0; trial < n_layout; trial++) {
        const Matrix M = random_matrix(rng);
        const int n_tx = M.n_tx, n_rows = M.n_rows;
        const std::vector<uint64_t> &rp = M.rp;
        const std::vector<int32_t> &ci = M.ci;
        if (trial % 4 == 1) setenv("EMSAR_HIP_FRAG_ROWS", "3072", 1);          // many independently tiled fragments, several threads
        else if (trial % 4 == 2) setenv("EMSAR_HIP_FRAG_ROWS", "7000", 1);
        else unsetenv("EMSAR_HIP_FRAG_ROWS");
        for (int merge = 0; merge < 2; merge++) {
            emsar::TiledLayout L, L1;
            setenv("EMSAR_HOST_THREADS", trial % 2 ? "5" : "16", 1);             // classification, both sorts and the fragments on several threads
            int rc = emsar::build_tiled(n_rows, n_tx, rp.data(), ci.data(), L, merge);
            int ck = rc ? -99 : emsar::check_tiled(L, rp.data(), ci.data());
            if (rc || ck) { printf("FAIL trial %d merge %d rc %d ck %d\n", trial, merge, rc, ck); return 1; }
            {                                                                    // what the unit kernel reads first, derived from the layout
                emsar::UnitTables U;
                emsar::build_unit_tables(L, U);
                const int cu = emsar::check_unit_tables(L, U);
                if (cu) { printf("FAIL trial %d merge %d unit tables %d\n", trial, merge, cu); return 1; }
            }
            if (!L.tiles.empty()) {                                              // a descriptor that points past its arrays must be caught on the host
                size_t last = 0;
                for (size_t i = 0; i < L.tiles.size(); i++) if (L.tiles[i].fwd_off > L.tiles[last].fwd_off) last = i;
                emsar::TiledLayout B = L;
                B.tiles[last].k[B.tiles[last].n_slices - 1] += 1;                  // one forward column more than was stored
                emsar::TiledLayout C = L;
                C.tiles[trial % C.tiles.size()].row_base += emsar::kTileSliceRows * 4;   // row slots of another tile, or past the end
                emsar::TiledLayout D = L;
                D.tiles[trial % D.tiles.size()].near_n = 0; D.tiles[trial % D.tiles.size()].far_n = 0;   // ids beyond the dictionary
                if (emsar::check_tiled_extents(B) == 0 || emsar::check_tiled_extents(C) == 0 || emsar::check_tiled_extents(D) == 0) {
                    printf("FAIL trial %d merge %d: a bad descriptor passed the extent check\n", trial, merge); return 1;
                }
            }
            setenv("EMSAR_HOST_THREADS", "1", 1);                                // the layout must not depend on the thread count
            rc = emsar::build_tiled(n_rows, n_tx, rp.data(), ci.data(), L1, merge);
            if (rc || !same_layout(L, L1)) { printf("FAIL trial %d merge %d: layout depends on the thread count\n", trial, merge); return 1; }
            unsetenv("EMSAR_HOST_THREADS");
        }
    }
    // set-resident records: sparse family-like matrices (many small sets), weights with zeros, a few huge rows
    for (int trial = 0; trial < n_sets; trial++) {
        int n_tx = 20 + rng() % 6000;
        int n_rows = rng() % 30000;
        int fam = 2 + rng() % (trial % 3 == 0 ? 400 : 12);
        std::vector<uint64_t> rp(1, 0);
        std::vector<int32_t> ci, w;
        for (int r = 0; r < n_rows; r++) {
            int k = rng() % 100 < 40 ? 1 : 1 + rng() % std::min(fam, 30);
            if (rng() % 60 == 0) k = 0;
            if (trial % 7 == 0 && rng() % 2000 == 0) k = 3000;
            int base = (int)(rng() % n_tx) / fam * fam;
            for (int j = 0; j < k; j++) ci.push_back(rng() % 400 == 0 ? (int)(rng() % n_tx) : std::min(n_tx - 1, base + (int)(rng() % fam)));
            rp.push_back(ci.size());
            w.push_back(rng() % 3 == 0 ? 0 : 1 + rng() % 50);
        }
        emsar::ResidentSets S;
        const int32_t *wp = trial % 5 == 4 ? nullptr : w.data();
        emsar::build_sets(n_rows, n_tx, rp.data(), ci.data(), wp, S);
        int ck = emsar::check_sets(n_rows, n_tx, rp.data(), ci.data(), wp, S);
        if (ck) { printf("FAIL sets trial %d ck %d\n", trial, ck); return 1; }
        if (S.n_closed_tids + S.n_resident_tids + S.n_streamed_tids + S.CL.n_tids != n_tx) { printf("FAIL sets census %d\n", trial); return 1; }
    }
    printf("ok\n");
    return 0;
}
