// chol16_order_check.hip — the instruction order of c16_solve (sadvio_amd/csrc/chol16.h) does not change its bits. The header requests
// the H column of a back-substitution step one step ahead; -DSADVIO_C16_PARENT_ORDER restores the loop that requested it in front of
// the step's own barrier. The floating-point operations and their order are the same.
// This program is built TWICE, with and without that macro; each build runs the sizes of chol16_tail_check.hip on the same
// seeded images (its own generator: see uniform01), with both tails, and writes to the file named by its argument, per size and tail:
//   N | old_tail | return value of SOLVE = true | xs[0 .. N) | return value of SOLVE = false | the whole image of SOLVE = false
// tests/test_gpu_chol16_order.py compares the two files byte for byte. Each build also checks, on its own,
//   * the solution against a host Cholesky solve (bound below),
//   * that a system with a non-positive pivot returns false,
// and ends with exit status 0 and a last line "chol16_order_check: OK" when both hold.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -munsafe-fp-atomics [-DSADVIO_C16_PARENT_ORDER] -o chol16_order_check tests/cpp/chol16_order_check.hip
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../sadvio_amd/csrc/chol16.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); exit(2); } } while (0)
using namespace sadvio;

#ifdef SADVIO_C16_PARENT_ORDER
static const char* ORDER = "parent order";
#else
static const char* ORDER = "product order";
#endif

// One workgroup: image -> LDS, symmetrize, solve; xs (SOLVE) and the whole image back
template <bool SOLVE>
__global__ __launch_bounds__(512) void k_check(const double* img, int N, double* xout, double* imgout, int* ok, int old_tail) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int nb = c16_blocks(N + 1);
    const int sz = c16_size(N);
    double* A = (double*)smem;
    double* pub = A + sz;
    double* yv = pub + C16_WORK;
    double* xs = yv + 16 * nb;       // 16 * nb + 16 doubles
    for (int i = threadIdx.x; i < sz; i += blockDim.x) A[i] = img[i];
    for (int i = threadIdx.x; i < 16 * nb + 16; i += blockDim.x) xs[i] = 0.0;
    __syncthreads();
    c16_symmetrize(A, nb);
    __syncthreads();
    const bool good = c16_solve<1, SOLVE>(A, N, xs, pub, yv, nullptr, nullptr, old_tail != 0);
    __syncthreads();
    for (int i = threadIdx.x; i < N; i += blockDim.x) xout[i] = xs[i];
    for (int i = threadIdx.x; i < sz; i += blockDim.x) imgout[i] = A[i];
    if (threadIdx.x == 0) *ok = good ? 1 : 0;
}

static bool host_solve(std::vector<double> S, std::vector<double> b, int N, std::vector<double>& x) {
    for (int j = 0; j < N; j++) {
        double d = S[j * N + j];
        for (int q = 0; q < j; q++) d -= S[j * N + q] * S[j * N + q];
        if (!(d > 0)) return false;
        d = sqrt(d); S[j * N + j] = d;
        for (int i = j + 1; i < N; i++) {
            double t = S[i * N + j];
            for (int q = 0; q < j; q++) t -= S[i * N + q] * S[j * N + q];
            S[i * N + j] = t / d;
        }
    }
    for (int i = 0; i < N; i++) { double t = b[i]; for (int q = 0; q < i; q++) t -= S[i * N + q] * b[q]; b[i] = t / S[i * N + i]; }
    for (int i = N - 1; i >= 0; i--) { double t = b[i]; for (int q = i + 1; q < N; q++) t -= S[q * N + i] * b[q]; b[i] = t / S[i * N + i]; }
    x = b;
    return true;
}

struct Run { std::vector<double> x, img; int ok; };

// The generator is the program's own: the two builds must draw the same images, and rand() is shared with whatever else the process
// runs between two sizes (its sequence came out differently in two runs of one binary once the HIP runtime was up).
static unsigned long long rng_state = 11;
static double uniform01() {      // splitmix64, the top 53 bits
    unsigned long long z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

template <bool SOLVE>
static Run run(const double* dimg, int N, int old_tail, double* dx, double* dout, int* dok) {
    const int sz = c16_size(N), nb = c16_blocks(N + 1);
    const size_t lds = (size_t)(sz + C16_WORK + 16 * nb + 16 * nb + 16) * 8;
    CK(hipFuncSetAttribute((const void*)k_check<SOLVE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    CK(hipMemset(dx, 0, (N + 1) * 8)); CK(hipMemset(dout, 0, sz * 8)); CK(hipMemset(dok, 0xff, 4));
    hipLaunchKernelGGL(k_check<SOLVE>, dim3(1), dim3(512), lds, 0, dimg, N, dx, dout, dok, old_tail);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    Run r; r.x.resize(N); r.img.resize(sz);
    CK(hipMemcpy(r.x.data(), dx, N * 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(r.img.data(), dout, sz * 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(&r.ok, dok, 4, hipMemcpyDeviceToHost));
    return r;
}

int main(int argc, char** argv) {
    if (argc != 2) { printf("usage: chol16_order_check OUTPUT_FILE\n"); return 2; }
    FILE* out = fopen(argv[1], "wb");
    if (!out) { printf("cannot write %s\n", argv[1]); return 2; }
    CK(hipSetDevice(0));
    // the sizes of chol16_tail_check.hip, images made the same way
    const int sizes[] = {1, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 80, 112, 113, 114, 127, 128, 129, 165, 174, -114};   // < 0: a non-positive pivot
    int fails = 0;
    for (int Ns : sizes) {
        const bool broken = Ns < 0;
        const int N = broken ? -Ns : Ns;
        std::vector<double> S((size_t)N * N), b(N), x, G((size_t)N * N);
        // S = G G^T / N + 0.05 I: dense, lambda_min >= 0.05
        for (auto& v : G) v = uniform01() - 0.5;
        for (int i = 0; i < N; i++)
            for (int j = 0; j <= i; j++) {
                double t = 0;
                for (int q = 0; q < N; q++) t += G[(size_t)i * N + q] * G[(size_t)j * N + q];
                S[(size_t)i * N + j] = S[(size_t)j * N + i] = t / N + (i == j ? 0.05 : 0.0);
            }
        for (auto& v : b) v = uniform01() - 0.5;
        if (broken) S[(size_t)70 * N + 70] = -1.0;   // inside block 4: the factorisation meets it, every later block carries the NaN
        const bool host_ok = host_solve(S, b, N, x);
        if (host_ok == broken) { printf("N=%d: host solve %s\n", N, host_ok ? "did not fail on the broken system" : "failed"); fails++; continue; }
        const int sz = c16_size(N);
        std::vector<double> img(sz, 0.0);
        for (int i = 0; i < N; i++) for (int j = 0; j <= i; j++) img[c16_index(i, j)] = S[(size_t)i * N + j];
        for (int j = 0; j < N; j++) img[c16_index(N, j)] = b[j];
        double *dimg, *dx, *dout; int* dok;
        CK(hipMalloc(&dimg, sz * 8)); CK(hipMalloc(&dx, (N + 1) * 8)); CK(hipMalloc(&dout, sz * 8)); CK(hipMalloc(&dok, 4));
        CK(hipMemcpy(dimg, img.data(), sz * 8, hipMemcpyHostToDevice));
        for (int old_tail = 0; old_tail < 2; old_tail++) {
            const Run s = run<true>(dimg, N, old_tail, dx, dout, dok), f = run<false>(dimg, N, old_tail, dx, dout, dok);
            fwrite(&N, sizeof(int), 1, out); fwrite(&old_tail, sizeof(int), 1, out);
            fwrite(&s.ok, sizeof(int), 1, out); fwrite(s.x.data(), 8, (size_t)N, out);
            fwrite(&f.ok, sizeof(int), 1, out); fwrite(f.img.data(), 8, (size_t)sz, out);
            if (broken) {
                const bool good = s.ok == 0;
                printf("N=%3d non-positive pivot, old_tail %d: returns %d  %s\n", N, old_tail, s.ok, good ? "ok" : "FAIL");
                if (!good) fails++;
                continue;
            }
            // Against the host: both are backward-stable Cholesky solves, each within (3 N + 1) eps kappa |x| of the exact solution to
            // first order (Higham, Accuracy and Stability, th. 10.4), so they differ by less than 8 N eps kappa max|x|, with
            // kappa <= |S|_inf / 0.05 (|S|_inf >= lambda_max, lambda_min >= 0.05)
            double err = 0, mx = 0, ninf = 0;
            for (int i = 0; i < N; i++) {
                err = fmax(err, fabs(s.x[i] - x[i])); mx = fmax(mx, fabs(x[i]));
                double rs = 0; for (int j = 0; j < N; j++) rs += fabs(S[(size_t)i * N + j]);
                ninf = fmax(ninf, rs);
            }
            const double tol = 8.0 * N * 2.220446049250313e-16 * (ninf / 0.05) * mx;
            const bool good = s.ok == 1 && f.ok == 1 && err <= tol;
            printf("N=%3d old_tail %d returns %d | %d, max|x - x_host| %.2e (bound %.2e, |x| %.2e)  %s\n", N, old_tail, s.ok, f.ok, err, tol, mx, good ? "ok" : "FAIL");
            if (!good) fails++;
        }
        CK(hipFree(dimg)); CK(hipFree(dx)); CK(hipFree(dout)); CK(hipFree(dok));
    }
    if (fclose(out) != 0) { printf("write error on %s\n", argv[1]); return 2; }
    if (fails) { printf("chol16_order_check (%s): %d FAILED\n", ORDER, fails); return 1; }
    printf("chol16_order_check: OK (%s)\n", ORDER);
    return 0;
}
