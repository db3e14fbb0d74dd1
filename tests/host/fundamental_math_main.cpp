// fundamental_math_main.cpp -- runs the __host__ __device__ functions of
// surfhip_fundamental_math.inc and surfhip_ransac_sample.inc on the CPU, for
// tests/test_fundamental_math_host.py.
//
//   fundamental_math_main <cases> <results>
//
// Both files are streams of little-endian records.  A case starts with an
// int32 opcode and an int32 count of items:
//   1 sample      per item uint32 seed, uint32 hyp, int32 n, int32 K (4 or 8) -> K int32
//   2 sampson2    per item 13 float32 (f[9], x, y, u, v)         -> 1 float32
//   3 eight_point per item 32 float64 (x[8], y[8], u[8], v[8])   -> int32 ok, 9 float32
//   4 jacobi      per item int32 n, n*n float64 (row-major A)    -> n*n float64 A, n*n float64 V
//   5 refit_solve per item 42 float64 (m[36], cx, cy, s1, cu, cv, s2) -> int32 ok, 9 float32
//   6 sample histogram: uint32 seed, int32 n, int32 nhyp, int32 K (4 or 8) (count = 1)
//                 -> n int64 hits per index, int32 bad (samples with a repeated or out-of-range index)
// Exit status 0 when every case was read and written.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#define __host__
#define __device__
#define __forceinline__ inline
using std::max;
using std::min;

namespace {
#include "surfhip_fundamental_math.inc"
#include "surfhip_ransac_sample.inc"

template <class T>
bool get(FILE* f, T* p, size_t n = 1)
{
    return fread(p, sizeof(T), n, f) == n;
}

template <class T>
bool put(FILE* f, const T* p, size_t n = 1)
{
    return fwrite(p, sizeof(T), n, f) == n;
}

template <int K>
bool sample_item(uint32_t seed, uint32_t hyp, int32_t n, FILE* out)
{
    if (n < K) return false;
    int idx[K];
    fd_sample<K>(seed, hyp, n, idx);
    int32_t o[K];
    for (int j = 0; j < K; ++j) o[j] = idx[j];
    return put(out, o, K);
}

template <int K>
bool sample_histogram(uint32_t seed, int32_t n, int32_t nhyp, FILE* out)
{
    if (n < K) return false;
    std::vector<int64_t> hits((size_t)n, 0);
    int32_t bad = 0;
    for (int32_t h = 0; h < nhyp; ++h) {
        int idx[K];
        fd_sample<K>(seed, (uint32_t)h, n, idx);
        bool ok = true;
        for (int j = 0; j < K; ++j) {
            ok = ok && idx[j] >= 0 && idx[j] < n;
            for (int i = 0; i < j; ++i) ok = ok && idx[i] != idx[j];
        }
        if (!ok) { ++bad; continue; }
        for (int j = 0; j < K; ++j) ++hits[(size_t)idx[j]];
    }
    return put(out, hits.data(), hits.size()) && put(out, &bad);
}

bool run_case(int op, int count, FILE* in, FILE* out)
{
    for (int it = 0; it < count; ++it) {
        if (op == 1) {
            uint32_t sh[2];
            int32_t nk[2];
            if (!get(in, sh, 2) || !get(in, nk, 2) || (nk[1] != 4 && nk[1] != 8)) return false;
            if (!(nk[1] == 4 ? sample_item<4>(sh[0], sh[1], nk[0], out) : sample_item<8>(sh[0], sh[1], nk[0], out)))
                return false;
        } else if (op == 2) {
            float a[13];
            if (!get(in, a, 13)) return false;
            const float e = fd_sampson2(a, a[9], a[10], a[11], a[12]);
            if (!put(out, &e)) return false;
        } else if (op == 3) {
            double x[8], y[8], u[8], v[8];
            if (!get(in, x, 8) || !get(in, y, 8) || !get(in, u, 8) || !get(in, v, 8)) return false;
            float f[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            const int32_t ok = fd_eight_point(x, y, u, v, f) ? 1 : 0;
            if (!put(out, &ok) || !put(out, f, 9)) return false;
        } else if (op == 4) {
            int32_t n;
            if (!get(in, &n) || n < 1 || n > 9) return false;
            std::vector<double> A((size_t)n * n), V((size_t)n * n);
            if (!get(in, A.data(), A.size())) return false;
            fd_jacobi(A.data(), V.data(), n, FdSolo{});
            if (!put(out, A.data(), A.size()) || !put(out, V.data(), V.size())) return false;
        } else if (op == 5) {
            double m[36], t[6], ws[180];
            if (!get(in, m, 36) || !get(in, t, 6)) return false;
            float f[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            const int32_t ok = fd_refit_solve(m, t[0], t[1], t[2], t[3], t[4], t[5], ws, f, FdSolo{}) ? 1 : 0;
            if (!put(out, &ok) || !put(out, f, 9)) return false;
        } else if (op == 6) {
            uint32_t seed;
            int32_t a[3];                               // n, nhyp, K
            if (!get(in, &seed) || !get(in, a, 3) || (a[2] != 4 && a[2] != 8)) return false;
            if (!(a[2] == 4 ? sample_histogram<4>(seed, a[0], a[1], out) : sample_histogram<8>(seed, a[0], a[1], out)))
                return false;
        } else {
            return false;
        }
    }
    return true;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: %s <cases> <results>\n", argv[0]);
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) {
        fprintf(stderr, "cannot open %s or %s\n", argv[1], argv[2]);
        return 2;
    }
    int32_t head[2];
    bool ok = true;
    while (ok && get(in, head, 2)) ok = run_case(head[0], head[1], in, out);
    ok = ok && feof(in);
    fclose(in);
    if (fclose(out) != 0) ok = false;
    if (!ok) fprintf(stderr, "malformed case file or short write\n");
    return ok ? 0 : 1;
}
