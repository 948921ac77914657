// chol16_tail_check.hip — the two tails of c16_solve (sadvio_amd/csrc/chol16.h) on the same images: the product's (the last block
// column without a barrier, its neighbour's panel turned into H one phase early, x_I loaded ahead of the back-substitution's FMAs)
// against old_tail (the last block column as every other one). Neither changes a floating-point operation or its order, so for seeded
// random SPD systems of every size at which the tail takes another path
//   * SOLVE = true:  xs is equal BIT FOR BIT and so is the return value,
//   * SOLVE = false: the whole returned image is equal bit for bit (what dense_chol.h takes from it),
//   * the solution agrees with a host Cholesky solve (bound below),
//   * a system with a non-positive pivot returns false from both.
// Exit status 0 and a last line "chol16_tail_check: OK" when all of it holds. tests/test_gpu_chol16_tail.py builds and runs it.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -munsafe-fp-atomics -o chol16_tail_check tests/cpp/chol16_tail_check.hip
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../sadvio_amd/csrc/chol16.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); exit(2); } } while (0)
using namespace sadvio;

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

int main() {
    CK(hipSetDevice(0));
    // one block with and without the right-hand side in its own tile row | two blocks: the first step of the back-substitution | three
    // and four blocks: one wave | the fifth block, in the next wave | config 2 and its neighbours | the ninth block | config 3 | the cap
    const int sizes[] = {1, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 80, 112, 113, 114, 127, 128, 129, 165, 174, -114};   // < 0: a non-positive pivot
    int fails = 0;
    srand(11);
    for (int Ns : sizes) {
        const bool broken = Ns < 0;
        const int N = broken ? -Ns : Ns;
        std::vector<double> S((size_t)N * N), b(N), x, G((size_t)N * N);
        // S = G G^T / N + 0.05 I: dense, lambda_min >= 0.05
        for (auto& v : G) v = (double)rand() / RAND_MAX - 0.5;
        for (int i = 0; i < N; i++)
            for (int j = 0; j <= i; j++) {
                double t = 0;
                for (int q = 0; q < N; q++) t += G[(size_t)i * N + q] * G[(size_t)j * N + q];
                S[(size_t)i * N + j] = S[(size_t)j * N + i] = t / N + (i == j ? 0.05 : 0.0);
            }
        for (auto& v : b) v = (double)rand() / RAND_MAX - 0.5;
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
        const Run sn = run<true>(dimg, N, 0, dx, dout, dok), so = run<true>(dimg, N, 1, dx, dout, dok);
        const Run fn = run<false>(dimg, N, 0, dx, dout, dok), fo = run<false>(dimg, N, 1, dx, dout, dok);
        CK(hipFree(dimg)); CK(hipFree(dx)); CK(hipFree(dout)); CK(hipFree(dok));
        const bool same_ret = sn.ok == so.ok && (sn.ok == 0 || sn.ok == 1);
        const bool same_img = memcmp(fn.img.data(), fo.img.data(), (size_t)sz * 8) == 0;
        if (broken) {
            const bool good = same_ret && sn.ok == 0 && same_img;
            printf("N=%3d non-positive pivot: new tail returns %d, old tail %d, SOLVE=false images %s  %s\n", N, sn.ok, so.ok, same_img ? "equal" : "DIFFER", good ? "ok" : "FAIL");
            if (!good) fails++;
            continue;
        }
        const bool same_x = memcmp(sn.x.data(), so.x.data(), (size_t)N * 8) == 0;
        // Against the host: both are backward-stable Cholesky solves, each within (3 N + 1) eps kappa |x| of the exact solution to
        // first order (Higham, Accuracy and Stability, th. 10.4), so they differ by less than 8 N eps kappa max|x|, with
        // kappa <= |S|_inf / 0.05 (|S|_inf >= lambda_max, lambda_min >= 0.05)
        double err = 0, mx = 0, ninf = 0;
        for (int i = 0; i < N; i++) {
            err = fmax(err, fabs(sn.x[i] - x[i])); mx = fmax(mx, fabs(x[i]));
            double rs = 0; for (int j = 0; j < N; j++) rs += fabs(S[(size_t)i * N + j]);
            ninf = fmax(ninf, rs);
        }
        const double tol = 8.0 * N * 2.220446049250313e-16 * (ninf / 0.05) * mx;
        const bool good = same_ret && sn.ok == 1 && same_x && same_img && err <= tol;
        printf("N=%3d returns %d | %d, xs %s, SOLVE=false image (%d doubles) %s, max|x - x_host| %.2e (bound %.2e, |x| %.2e)  %s\n", N, sn.ok, so.ok,
               same_x ? "bit-equal" : "DIFFER", sz, same_img ? "bit-equal" : "DIFFER", err, tol, mx, good ? "ok" : "FAIL");
        if (!good) fails++;
    }
    if (fails) { printf("chol16_tail_check: %d FAILED\n", fails); return 1; }
    printf("chol16_tail_check: OK\n");
    return 0;
}
