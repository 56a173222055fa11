// Stand-alone check of the host Tile_create and tilespmv_cpu on CSR input that stores the same (i, j) more than once (tests/dup_cases.py has the same planted tiles).
// DNS, DNSROW and DNSCOL hold one value per position; chosen from entry COUNTS, they lose values (100 positions stored twice "fill" a tile by 75 %: the last duplicate
// wins) or are written past their slots (a row of 16 columns stored twice: 48 values into 16 slots; a column of 8 rows stored twice: 16 column ids into 1).  A tile with a
// repeated position must get COO, ELL, HYB or CSR, and y is the sum over all stored entries.  Built and run by tests/test_dup_cases_cpu.py with AddressSanitizer and UBSan
// on the host side, for both value types: Tile_create_ex (flags 0, HYB, CDNA4, TRANSPOSE) and tilespmv_cpu on every case, y compared with a CSR loop in integers.  Every
// array is exactly as long as the header says, so the sanitizer sees every step past it.  Values k / 16 and integer x in fp64, small integers in fp32: exact in any order.
// Exit status 0 = everything holds; every failure is printed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "tilespmv.h"

struct Case { const char *name; int rows, cols; std::vector<std::pair<int, int>> ent; bool positional_ok; };   // entries (i, j), repeats included

static uint64_t lcg(uint64_t &s) { s = s * 6364136223846793005ull + 1442695040888963407ull; return s >> 33; }

static void rep(Case &c, int i, int j, int times) { for (int k = 0; k < times; k++) c.ent.push_back({i, j}); }

static std::vector<Case> make_cases()
{
    std::vector<Case> v;
    { Case c{"A: 100 positions of a 16 x 16 tile, each stored twice", 16, 16, {}, false}; for (int k = 0; k < 100; k++) { const int p = (k * 37) & 255; rep(c, p >> 4, p & 15, 2); } v.push_back(c); }
    { Case c{"B: one row, 8 columns stored twice", 16, 16, {}, false}; for (int j = 0; j < 8; j++) rep(c, 3, 2 * j, 2); v.push_back(c); }
    { Case c{"B's column twin: one column, 8 rows stored twice", 16, 16, {}, false}; for (int i = 0; i < 8; i++) rep(c, 2 * i + 1, 5, 2); v.push_back(c); }
    { Case c{"D: one row of 16 columns stored twice, one full row", 16, 16, {}, false}; for (int j = 0; j < 16; j++) { rep(c, 2, j, 2); rep(c, 9, j, 1); } v.push_back(c); }
    { Case c{"D's column twin: one column of 16 rows stored twice, one full column", 16, 16, {}, false}; for (int i = 0; i < 16; i++) { rep(c, i, 4, 2); rep(c, i, 11, 1); } v.push_back(c); }
    { Case c{"F: 5 x 7 matrix, 14 positions stored twice", 5, 7, {}, false}; for (int k = 0; k < 14; k++) { const int p = (k * 12) % 35; rep(c, p / 7, p % 7, 2); } v.push_back(c); }
    { Case c{"G: one column, rows 0 .. 7 stored twice", 16, 16, {}, false}; for (int i = 0; i < 8; i++) rep(c, i, 6, 2); v.push_back(c); }
    { Case c{"G's row twin: one row, columns 0 .. 7 stored twice", 16, 16, {}, false}; for (int j = 0; j < 8; j++) rep(c, 0, j, 2); v.push_back(c); }
    { Case c{"four columns of one row stored four times", 16, 16, {}, false}; for (int j = 0; j < 4; j++) rep(c, 7, 3 * j, 4); v.push_back(c); }
    { Case c{"four rows of one column stored four times", 16, 16, {}, false}; for (int i = 0; i < 4; i++) rep(c, 3 * i, 15, 4); v.push_back(c); }
    {   // ragged rows, 255 entries: the most a tile with repeats serves (its row pointer is bytes)
        Case c{"255 entries in ragged rows", 16, 16, {}, false};
        const int counts[16] = {45, 5, 40, 5, 35, 5, 30, 5, 25, 5, 20, 5, 15, 5, 5, 5};
        for (int r = 0; r < 16; r++) for (int k = 0; k < counts[r]; k++) rep(c, r, (5 * k + r) & 15, 1);
        v.push_back(c);
    }
    { Case c{"a full 16 x 16 tile without repeats (stays dense)", 16, 16, {}, true}; for (int p = 0; p < 256; p++) rep(c, p >> 4, p & 15, 1); v.push_back(c); }
    return v;
}

static int run(const Case &c, unsigned flags, const char *flag_name)
{
    const bool f32 = sizeof(MAT_VAL_TYPE) == 4, tr = (flags & TILESPMV_CREATE_TRANSPOSE) != 0;
    const int rows = c.rows, cols = c.cols, kmax = f32 ? 15 : 1023, xmax = f32 ? 63 : (1 << 20), den = f32 ? 1 : 16;
    const int nnz = (int)c.ent.size(), out_rows = tr ? cols : rows, in_cols = tr ? rows : cols;
    uint64_t seed = 97u + (uint64_t)nnz * 7919u;
    // CSR with the entries of every row in shuffled order: repeats are not adjacent
    std::vector<MAT_PTR_TYPE> rp(rows + 1, 0);
    std::vector<int> ci(nnz);
    for (const auto &e : c.ent) rp[e.first + 1]++;
    for (int r = 0; r < rows; r++) rp[r + 1] += rp[r];
    { std::vector<int> at(rp.begin(), rp.end() - 1); for (const auto &e : c.ent) ci[at[e.first]++] = e.second; }
    for (int r = 0; r < rows; r++)
        for (int k = rp[r + 1] - 1; k > rp[r]; k--) std::swap(ci[k], ci[rp[r] + (int)(lcg(seed) % (uint64_t)(k - rp[r] + 1))]);
    std::vector<long long> kv(nnz), kx(in_cols), sum(out_rows, 0);
    std::vector<MAT_VAL_TYPE> v(nnz), x(in_cols), y(out_rows), gold(out_rows);
    for (int i = 0; i < nnz; i++) { kv[i] = (long long)(1 + lcg(seed) % kmax) * (lcg(seed) & 1 ? 1 : -1); v[i] = (MAT_VAL_TYPE)kv[i] / (MAT_VAL_TYPE)den; }
    for (int j = 0; j < in_cols; j++) { kx[j] = (long long)(1 + lcg(seed) % xmax) * (lcg(seed) & 1 ? 1 : -1); x[j] = (MAT_VAL_TYPE)kx[j]; }
    for (int r = 0; r < rows; r++)
        for (int k = rp[r]; k < rp[r + 1]; k++) { if (tr) sum[ci[k]] += kv[k] * kx[r]; else sum[r] += kv[k] * kx[ci[k]]; }
    for (int r = 0; r < out_rows; r++) gold[r] = (MAT_VAL_TYPE)sum[r] / (MAT_VAL_TYPE)den;
    int bad = 0;
    Tile_matrix T;
    Tile_create_ex(&T, rows, cols, nnz, rp.data(), ci.data(), v.data(), flags | TILESPMV_CREATE_QUIET);
    for (int t = 0; t < T.tilenum; t++) {
        const int f = T.Format[t];
        const bool positional = f == TILESPMV_FMT_DNS || f == TILESPMV_FMT_DNSROW || f == TILESPMV_FMT_DNSCOL;
        if (positional != c.positional_ok) { printf("%s [%s, %s]: tile %d has format %d\n", c.name, flag_name, f32 ? "f32" : "f64", t, f); bad++; }
    }
    std::vector<int> p1(T.tilenum + 1), p2(T.tilenum + 1);
    int nblk = 0; unsigned int *a = nullptr; int *b = nullptr, *d = nullptr;
    for (auto &e : y) e = (MAT_VAL_TYPE)-7;
    tilespmv_cpu(&T, p1.data(), p2.data(), &nblk, &a, &b, &d, out_rows, in_cols, nnz, rp.data(), ci.data(), v.data(), x.data(), y.data(), gold.data());
    free(a); free(b); free(d);
    int wrong = 0;
    for (int r = 0; r < out_rows; r++) wrong += y[r] != gold[r];
    if (wrong) { printf("%s [%s, %s]: %d rows of y are wrong\n", c.name, flag_name, f32 ? "f32" : "f64", wrong); bad++; }
    Tile_destroy(&T);
    return bad ? 1 : 0;
}

int main()
{
    const std::vector<Case> cases = make_cases();
    const struct { unsigned flags; const char *name; } sets[] = {{0u, "plain"}, {TILESPMV_CREATE_HYB, "hyb"}, {TILESPMV_CREATE_CDNA4, "cdna4"}, {TILESPMV_CREATE_TRANSPOSE, "transpose"}};
    int bad = 0, n = 0;
    for (const Case &c : cases)
        for (const auto &s : sets) { bad += run(c, s.flags, s.name); n++; }
    printf("%d cases, %d failures\n", n, bad);
    return bad ? 1 : 0;
}
