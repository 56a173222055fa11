// Stand-alone check of the host Tile_create and tilespmv_cpu on short, wide matrices whose HYB tiles sit in a partial last tile-row (tests/hyb_cases.py has the same matrices):
// every such tile of odd width and odd height takes half a byte of hybIdx more than (hybellsize + 1) / 2 + hybcoosize allows, so an array of that size is too short — by 20 bytes
// for the 15 x 640 matrix, by 125 for the 11 x 4000 one.  Built and run by tests/test_hyb_idx_size_cpu.py with AddressSanitizer and UBSan on the host side, for both value
// types: Tile_create_ex (HYB rule on), tilespmv_cpu, then tilespmv_matrix_save / _load into argv[1] and tilespmv_cpu again, y compared each time with a CSR product in integers.
// The data is exact in any order: values k / 16 and integer x in fp64, small integers in fp32.  Exit status 0 = everything holds; every failure is printed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "tilespmv.h"

struct Case { int rows, blocks; std::vector<int> counts; int hyb_tiles, idx_bytes; };   // every block column holds one tile: row r has counts[r] entries in local columns 0 .. counts[r] - 1

static uint64_t lcg(uint64_t &s) { s = s * 6364136223846793005ull + 1442695040888963407ull; return s >> 33; }

static int run(const Case &c, const std::string &dir)
{
    const bool f32 = sizeof(MAT_VAL_TYPE) == 4;
    const int rows = c.rows, cols = 16 * c.blocks, kmax = f32 ? 15 : 1023, xmax = f32 ? 63 : (1 << 20), den = f32 ? 1 : 16;
    std::vector<MAT_PTR_TYPE> rp(rows + 1, 0);
    std::vector<int> ci;
    for (int r = 0; r < rows; r++) {
        for (int b = 0; b < c.blocks; b++)
            for (int k = 0; k < c.counts[r]; k++) ci.push_back(16 * b + k);
        rp[r + 1] = (MAT_PTR_TYPE)ci.size();
    }
    const int nnz = (int)ci.size();
    uint64_t seed = 12345u + (uint64_t)rows * 7919u;
    std::vector<long long> kv(nnz), kx(cols);
    std::vector<MAT_VAL_TYPE> v(nnz), x(cols), y(rows), gold(rows);   // (exactly as long as the header says: the sanitizer sees every step past them)
    for (int i = 0; i < nnz; i++) { kv[i] = (long long)(1 + lcg(seed) % kmax) * (lcg(seed) & 1 ? 1 : -1); v[i] = (MAT_VAL_TYPE)kv[i] / (MAT_VAL_TYPE)den; }
    for (int j = 0; j < cols; j++) { kx[j] = (long long)(1 + lcg(seed) % xmax) * (lcg(seed) & 1 ? 1 : -1); x[j] = (MAT_VAL_TYPE)kx[j]; }
    for (int r = 0; r < rows; r++) {
        long long s = 0;
        for (int k = rp[r]; k < rp[r + 1]; k++) s += kv[k] * kx[ci[k]];
        gold[r] = (MAT_VAL_TYPE)s / (MAT_VAL_TYPE)den;
    }
    int bad = 0;
    Tile_matrix T;
    Tile_create_ex(&T, rows, cols, nnz, rp.data(), ci.data(), v.data(), TILESPMV_CREATE_HYB | TILESPMV_CREATE_QUIET);
    int hyb = 0;
    for (int t = 0; t < T.tilenum; t++) hyb += T.Format[t] == TILESPMV_FMT_HYB;
    if (hyb != c.hyb_tiles) { printf("%d x %d: %d HYB tiles, expected %d\n", rows, cols, hyb, c.hyb_tiles); bad++; }
    const std::string path = dir + "/hyb_" + std::to_string(rows) + "x" + std::to_string(cols) + (f32 ? ".tile_f32" : ".tile_f64");
    for (int pass = 0; pass < 2; pass++) {
        Tile_matrix L; Tile_matrix *M = &T;
        if (pass == 1) {
            int r2 = 0, c2 = 0; MAT_PTR_TYPE z2 = 0;
            if (tilespmv_matrix_save(&T, rows, cols, nnz, path.c_str()) != 0 || tilespmv_matrix_load(&L, &r2, &c2, &z2, path.c_str()) != 0 || r2 != rows || c2 != cols || z2 != nnz) {
                printf("%d x %d: cache round trip failed\n", rows, cols); bad++; break;
            }
            M = &L;
        }
        std::vector<int> p1(T.tilenum + 1), p2(T.tilenum + 1);
        int nblk = 0; unsigned int *a = nullptr; int *b = nullptr, *d = nullptr;
        for (auto &e : y) e = (MAT_VAL_TYPE)-7;
        tilespmv_cpu(M, p1.data(), p2.data(), &nblk, &a, &b, &d, rows, cols, nnz, rp.data(), ci.data(), v.data(), x.data(), y.data(), gold.data());
        free(a); free(b); free(d);
        int wrong = 0, last = 0;
        for (int r = 0; r < rows; r++) wrong += y[r] != gold[r];
        for (int t = 0; t < M->tilenum; t++) if (M->Format[t] == TILESPMV_FMT_HYB) last = p2[t] + ((int)M->tilewidth[t] * (rows % 16 ? rows % 16 : 16) + 1) / 2 + (M->hyb_coocount[t + 1] - M->hyb_coocount[t]);
        if (wrong) { printf("%d x %d, %s: %d rows of y are wrong\n", rows, cols, pass ? "loaded from the cache" : "fresh", wrong); bad++; }
        if (last != c.idx_bytes) { printf("%d x %d, %s: the last HYB tile ends at byte %d of hybIdx, expected %d\n", rows, cols, pass ? "loaded from the cache" : "fresh", last, c.idx_bytes); bad++; }
        if (pass == 1) Tile_destroy(&L);
    }
    Tile_destroy(&T);
    remove(path.c_str());
    return bad;
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s <directory for the cache files>\n", argv[0]); return 2; }
    const Case cases[] = {
        {15, 40, {5, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0}, 40, 480},      // 40 HYB tiles of width 1, 15 rows high (8 bytes) + 4 remainder entries
        {11, 250, {5, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0}, 250, 2500},               // 250 HYB tiles of width 1, 11 rows high (6 bytes) + 4 remainder entries: a HYB tile in every block column of 4000
        {5, 250, {5, 1, 1, 1, 1}, 0, 0},                                      // 5 x 4000: no tile of 5 rows can pass the HYB rule (it wants 13 entries with at most 4 outside equal-width rows): no byte of hybIdx
    };
    int bad = 0;
    for (const Case &c : cases) bad += run(c, argv[1]);
    printf("%d cases, %d failures\n", (int)(sizeof(cases) / sizeof(*cases)), bad);
    return bad ? 1 : 0;
}
