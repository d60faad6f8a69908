// Dense coarse-inverse harness (k_gj_pinv0 + k_gj_step): random SPD E of size m with a wide diagonal scaling,
// checks max |D^-1 (E Einv - I) D| and reports the device time per inversion.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/bench_dense.hip -o tools/bench_dense && tools/bench_dense 567
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../instantsfm_amd/csrc/ba_gj.h"

using namespace insfm;

#define CK(x)                                                                           \
    do {                                                                                \
        hipError_t e_ = (x);                                                            \
        if (e_ != hipSuccess) { std::printf("%s: %s\n", #x, hipGetErrorString(e_)); std::exit(1); } \
    } while (0)

int main(int argc, char** argv) {
    const int m = argc > 1 ? std::atoi(argv[1]) : 567;
    const int reps = argc > 2 ? std::atoi(argv[2]) : 20;
    if (m < 1 || m > 4096) { std::printf("m out of range\n"); return 2; }
    std::mt19937_64 rng(1);
    std::normal_distribution<double> nd;
    std::vector<double> B((size_t)m * m), E((size_t)m * m, 0.0), sc(m);
    for (auto& v : B) v = nd(rng);
    for (int i = 0; i < m; ++i) sc[i] = std::pow(10.0, 4.0 * i / std::max(1, m - 1));
    for (int i = 0; i < m; ++i)
        for (int j = 0; j <= i; ++j) {
            double s = 0.0;
            for (int k = 0; k < m; ++k) s += B[(size_t)i * m + k] * B[(size_t)j * m + k];
            if (i == j) s += 1e-3 * m;
            E[(size_t)i * m + j] = E[(size_t)j * m + i] = s * sc[i] * sc[j];
        }
    const int nB = gj_steps(m), ld = nB * kGB;
    std::vector<double> Ep((size_t)ld * ld, 0.0), dh(ld, 1.0);
    for (int i = 0; i < ld; ++i)
        for (int j = 0; j < ld; ++j) Ep[(size_t)i * ld + j] = (i < m && j < m) ? E[(size_t)i * m + j] : (i == j ? 1.0 : 0.0);
    for (int i = 0; i < m; ++i) dh[i] = 1.0 / std::sqrt(E[(size_t)i * m + i]);
    double *dE, *dA, *dW, *dX, *dd, *dP;
    int* dok;
    CK(hipMalloc(&dE, sizeof(double) * ld * ld));
    CK(hipMalloc(&dA, sizeof(double) * ld * ld));
    CK(hipMalloc(&dW, sizeof(double) * ld * ld));
    CK(hipMalloc(&dX, sizeof(double) * m * m));
    CK(hipMalloc(&dd, sizeof(double) * ld));
    CK(hipMalloc(&dP, sizeof(double) * 2 * kGB * kGB));
    CK(hipMalloc(&dok, sizeof(int)));
    CK(hipMemcpy(dE, Ep.data(), sizeof(double) * ld * ld, hipMemcpyHostToDevice));
    CK(hipMemcpy(dd, dh.data(), sizeof(double) * ld, hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    float tot = 0.f;
    for (int r = 0; r < reps; ++r) {
        CK(hipMemcpy(dA, dE, sizeof(double) * ld * ld, hipMemcpyDeviceToDevice));
        CK(hipEventRecord(e0, nullptr));
        for (int u = 0; u <= nB; ++u) launch_gj_unit(u, m, dA, dW, dP, dd, dX, dok, nullptr);
        CK(hipEventRecord(e1, nullptr));
        CK(hipEventSynchronize(e1));
        float ms;
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (r >= 2) tot += ms;
    }
    int ok = 0;
    CK(hipMemcpy(&ok, dok, sizeof(int), hipMemcpyDeviceToHost));
    std::vector<double> X((size_t)m * m);
    CK(hipMemcpy(X.data(), dX, sizeof(double) * m * m, hipMemcpyDeviceToHost));
    double err = 0.0;
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) {
            double s = 0.0;
            for (int k = 0; k < m; ++k) s += E[(size_t)i * m + k] * X[(size_t)k * m + j];
            s -= (i == j) ? 1.0 : 0.0;
            err = std::max(err, std::fabs(s) * sc[j] / sc[i]);
        }
    unsigned long long hx = 1469598103934665603ull;  // FNV-1a of the result's bits: equal across bitwise-equal variants
    for (double v : X) {
        unsigned long long b;
        std::memcpy(&b, &v, sizeof b);
        hx = (hx ^ b) * 1099511628211ull;
    }
    std::printf("m=%d ok=%d max|D^-1(E Einv - I)D|=%.3e  %.1f us per inverse (%d launches)  bits %016llx\n", m, ok, err,
                1e3 * tot / std::max(1, reps - 2), nB + 1, hx);
    return (ok && err < 1e-6) ? 0 : 1;
}
