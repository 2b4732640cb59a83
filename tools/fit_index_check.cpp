// Stand-alone host-side check of the model fit's transposed index (emsar_amd/csrc/fit_index.hpp), meant to be compiled with
// -fsanitize=address,undefined and run on the CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/fit_index_check.cpp -o fit_index_check && ./fit_index_check
// A staircase of chunk sizes (transcripts that own 1, 255, 256, 257, 512, 513, 16 384 and 16 385 entries in rows {t, filler}, a few
// {t, t, filler}, among empty rows, in shuffled order) plus transcripts without entries goes through build_fit_index; the index is
// decoded again and compared with the rows, the padding bound is checked, and the walk of every chunk (fit_row_terms,
// fit_walk_chunk, fit_finish, fit_totals_host) runs over it once.
#include "../emsar_amd/csrc/fit_index.hpp"
#include <cstdio>
#include <cstdlib>
#include <random>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "fit_index_check: %s failed (line %d)\n", #c, __LINE__); return 1; } } while (0)

int main() {
    const int stairs[] = {1, 255, 256, 257, 512, 513, 64 * 256, 64 * 256 + 1};
    const int n_stairs = 8, n_fill = 300, n_tx = n_stairs + n_fill + 5;      // the last five own nothing
    std::mt19937 rng(11);
    std::vector<std::vector<int32_t>> rows;
    for (int t = 0; t < n_stairs; t++)
        for (int left = stairs[t]; left > 0;) {
            const int k = left >= 2 && rng() % 50 == 0 ? 2 : 1;
            std::vector<int32_t> row(k, t);
            row.insert(rng() % 3 ? row.end() : row.begin(), (int32_t)(n_stairs + rng() % n_fill));
            rows.push_back(row);
            left -= k;
        }
    for (int i = 0; i < 200; i++) rows.emplace_back();
    std::shuffle(rows.begin(), rows.end(), rng);
    const int64_t n_rows = (int64_t)rows.size();
    std::vector<uint64_t> rp(1, 0);
    std::vector<int32_t> ci;
    for (const auto &r : rows) { ci.insert(ci.end(), r.begin(), r.end()); rp.push_back(ci.size()); }
    const int64_t nnz = (int64_t)ci.size();

    emsar::FitIndex X;
    CHECK(emsar::build_fit_index(n_rows, n_tx, rp.data(), ci.data(), X) == 0);
    CHECK(X.index_slots() >= nnz && X.index_slots() <= nnz + 64 * 255);
    CHECK(X.n_groups == (X.n_chunks + 63) / 64 && (int64_t)X.chunk_tid.size() == X.n_chunks && (int64_t)X.chunk_out.size() == X.n_chunks);
    // decode: chunk by chunk in original order, a transcript's rows must come back in (row, position) order
    std::vector<std::vector<int32_t>> want(n_tx), got(n_tx);
    for (int64_t r = 0; r < n_rows; r++) for (uint64_t k = rp[r]; k < rp[r + 1]; k++) want[ci[k]].push_back((int32_t)r);
    std::vector<int64_t> sorted_of(X.n_chunks, -1);              // original chunk number -> sorted position, for the chunks of multi transcripts
    std::vector<int64_t> len(X.n_chunks, 0);
    int64_t used = 0;
    for (int64_t s = 0; s < X.n_chunks; s++) {
        const int64_t g = s / 64, base = X.group_base[g] + s % 64;
        int32_t j = 0;
        while (j < X.group_steps[g] && X.idx[base + 64 * (int64_t)j] >= 0) j++;
        for (int32_t k = j; k < X.group_steps[g]; k++) CHECK(X.idx[base + 64 * (int64_t)k] == -1);
        len[s] = j; used += j;
        CHECK(j <= emsar::kFitChunk);
        if (s > 0 && s % 64) CHECK(len[s] <= len[s - 1]);        // sorted by length inside a group (and across: the steps descend)
        if (X.chunk_out[s] >= 0) {
            CHECK(X.chunk_out[s] == X.chunk_tid[s]);
            for (int32_t k = 0; k < j; k++) got[X.chunk_tid[s]].push_back(X.idx[base + 64 * (int64_t)k]);
        } else {
            CHECK(-1 - (int64_t)X.chunk_out[s] < X.n_chunks);
            sorted_of[-1 - X.chunk_out[s]] = s;
        }
    }
    CHECK(used == nnz);
    for (int64_t g = 1; g < X.n_groups; g++) CHECK(X.group_steps[g] <= X.group_steps[g - 1]);
    CHECK(X.n_multi == 5);                                       // 257, 512, 513, 16 384, 16 385
    for (int64_t i = 0; i < X.n_multi; i++) {
        const int32_t t = X.multi[3 * i];
        for (int32_t c = X.multi[3 * i + 1]; c < X.multi[3 * i + 2]; c++) {
            const int64_t s = sorted_of[c];
            CHECK(s >= 0 && X.chunk_tid[s] == t);
            if (c + 1 < X.multi[3 * i + 2]) CHECK(len[s] == emsar::kFitChunk);
            const int64_t base = X.group_base[s / 64] + s % 64;
            for (int64_t k = 0; k < len[s]; k++) got[t].push_back(X.idx[base + 64 * k]);
        }
    }
    for (int t = 0; t < n_tx; t++) CHECK(got[t] == want[t]);

    // one walk over everything, as the host function does it
    std::vector<double> theta(n_tx);
    for (auto &v : theta) v = rng() % 5 ? (double)(rng() % 1000) / 37.0 : 0.0;
    std::vector<emsar::FitRec> rec(n_rows);
    for (int64_t c = 0; c < n_rows; c++) {
        emsar::FitRec x = {0, 0, 0, 0};
        double mu = 0, S = 0;
        if (rp[c] < rp[c + 1]) {
            for (uint64_t k = rp[c]; k < rp[c + 1]; k++) S = S + theta[ci[k]];
            x.S = emsar::fit_row_terms((double)(rng() % 40), 0.5 + (double)(rng() % 100) / 64.0, S, &mu, &x.q, &x.d, &x.a);
        }
        rec[c] = x;
    }
    std::vector<double> part(5 * X.n_chunks, 0.0), df(n_tx, 0.0);
    std::vector<int32_t> part_row(X.n_chunks, -1);
    for (int64_t s = 0; s < X.n_chunks; s++) {
        const emsar::FitAcc A = emsar::fit_walk_chunk(X.idx.data(), X.group_base[s / 64] + s % 64, X.group_steps[s / 64], theta[X.chunk_tid[s]], rec.data());
        if (X.chunk_out[s] >= 0) df[X.chunk_out[s]] = A.df;
        else {
            const int64_t k = -1 - (int64_t)X.chunk_out[s];
            part[k] = A.chi2; part[X.n_chunks + k] = A.dev; part[2 * X.n_chunks + k] = A.miss; part[3 * X.n_chunks + k] = A.df; part[4 * X.n_chunks + k] = A.best;
            part_row[k] = A.row;
        }
    }
    for (int64_t i = 0; i < X.n_multi; i++)
        df[X.multi[3 * i]] = emsar::fit_finish(part.data(), part_row.data(), X.n_chunks, X.multi[3 * i + 1], X.multi[3 * i + 2]).df;
    double tot[4], sum_df = 0.0, rows_reached = 0.0;
    emsar::fit_totals_host(rec.data(), n_rows, tot);
    for (double v : df) sum_df += v;
    for (const auto &x : rec) rows_reached += x.S > 0.0;
    CHECK(std::fabs(sum_df - rows_reached) <= 1e-9 * rows_reached);      // the shares of a row sum to one

    const long long chunks = (long long)X.n_chunks, slots = (long long)X.index_slots();

    // edge cases: no rows, one row, one transcript
    const uint64_t rp0[1] = {0}, rp1[2] = {0, 3};
    const int32_t c1[3] = {0, 0, 0};
    CHECK(emsar::build_fit_index(0, 3, rp0, nullptr, X) == 0 && X.n_chunks == 3 && X.index_slots() == 0);
    CHECK(emsar::build_fit_index(1, 1, rp1, c1, X) == 0 && X.n_chunks == 1 && X.index_slots() == 64 * 3);
    printf("fit_index_check ok: %lld rows, %lld entries, %lld chunks, %lld slots (%lld padding), %g infeasible rows\n", (long long)n_rows,
           (long long)nnz, chunks, slots, slots - (long long)nnz, tot[3]);
    return 0;
}
