// GPU check: ppm::atan2_unit (k_cand's wide-turn atan2, no special-case fallback) returns the same
// bits as ppm::atan2_fast for finite (y, x), not both zero, and NaN for NaN. Inputs: random unit
// vectors over every direction, random pairs over many binades, and the edge cases (signed zeros,
// |y/x| beyond 2^+-60, subnormals, the interval boundaries 7/16, 11/16, 19/16, 39/16).
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -std=c++17 -I../carnd-path-planning-project_amd/csrc
// Usage: atan2_check [nu]: nu inputs in each of the two large random sections and nu / 4 near the
// interval boundaries (default 2^24). Exit status 0 iff every input agrees.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <vector>
#include "pp_math.h"

__global__ void k_check(const double* y, const double* x, int n, unsigned long long* bad, double* ex) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double a = ppm::atan2_fast(y[i], x[i]);
    const double b = ppm::atan2_unit(y[i], x[i]);
    const bool same = (__double_as_longlong(a) == __double_as_longlong(b)) || (a != a && b != b);
    if (!same) {
        const unsigned long long k = atomicAdd(bad, 1ull);
        if (k < 8) { ex[4 * k] = y[i]; ex[4 * k + 1] = x[i]; ex[4 * k + 2] = a; ex[4 * k + 3] = b; }
    }
}

static uint64_t rng = 0x9E3779B97F4A7C15ull;
static uint64_t next() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; }
static double uni() { return (next() >> 11) * 0x1p-53; }

int main(int argc, char** argv) {
    std::vector<double> ys, xs;
    const double specials[] = {0.0, -0.0, 1.0, -1.0, 0x1p-61, -0x1p-61, 0x1p-70, 5e-324, -5e-324,
                               1e-300, 0x1p-1022, 7.0 / 16, 11.0 / 16, 19.0 / 16, 39.0 / 16, 0.5,
                               std::nextafter(7.0 / 16, 0.0), std::nextafter(11.0 / 16, 1.0), 1e300,
                               std::nan("")};
    for (double a : specials)
        for (double b : specials) {
            if (a == 0 && b == 0) continue;      // both zero: outside atan2_unit's domain
            for (int sa = -1; sa <= 1; sa += 2)
                for (int sb = -1; sb <= 1; sb += 2) { ys.push_back(sa * a); xs.push_back(sb * b); }
        }
    int nu = 1 << 24;
    if (argc > 1) {
        const long v = atol(argv[1]);
        if (v < 4 || v > (1 << 24)) { fprintf(stderr, "nu must be in [4, 2^24]\n"); return 2; }
        nu = (int)v;
    }
    for (int i = 0; i < nu; i++) {                 // unit vectors (the loop's inputs)
        const double t = (uni() * 2 - 1) * M_PI;
        ys.push_back(std::sin(t)); xs.push_back(std::cos(t));
    }
    for (int i = 0; i < nu; i++) {                 // ratios over many binades
        const double m1 = uni() + 0.5, m2 = uni() + 0.5;
        const int e1 = (int)(next() % 160) - 80, e2 = (int)(next() % 8) - 4;
        ys.push_back(std::ldexp(m1, e1) * ((next() & 1) ? 1 : -1));
        xs.push_back(std::ldexp(m2, e2) * ((next() & 1) ? 1 : -1));
    }
    for (int i = 0; i < nu / 4; i++) {             // near the interval boundaries
        const double r[] = {7.0 / 16, 11.0 / 16, 19.0 / 16, 39.0 / 16};
        const double x = uni() + 0.25;
        double y = x * r[next() & 3];
        const int k = (int)(next() % 9) - 4;
        for (int j = 0; j < std::abs(k); j++) y = std::nextafter(y, k > 0 ? 10.0 : 0.0);
        ys.push_back((next() & 1) ? y : -y); xs.push_back((next() & 1) ? x : -x);
    }
    const int n = (int)ys.size();
    double *dy, *dx, *dex;
    unsigned long long* dbad;
    hipMalloc(&dy, n * 8); hipMalloc(&dx, n * 8); hipMalloc(&dex, 32 * 8); hipMalloc(&dbad, 8);
    hipMemcpy(dy, ys.data(), n * 8, hipMemcpyHostToDevice);
    hipMemcpy(dx, xs.data(), n * 8, hipMemcpyHostToDevice);
    hipMemset(dbad, 0, 8);
    hipLaunchKernelGGL(k_check, dim3((n + 255) / 256), dim3(256), 0, 0, dy, dx, n, dbad, dex);
    unsigned long long bad = 0;
    double ex[32];
    hipMemcpy(&bad, dbad, 8, hipMemcpyDeviceToHost);
    hipMemcpy(ex, dex, sizeof ex, hipMemcpyDeviceToHost);
    printf("atan2_unit vs atan2_fast: %d inputs, %llu differ\n", n, bad);
    for (unsigned long long k = 0; k < bad && k < 8; k++)
        printf("  y=%a x=%a fast=%a unit=%a\n", ex[4 * k], ex[4 * k + 1], ex[4 * k + 2], ex[4 * k + 3]);
    return bad == 0 ? 0 : 1;
}
