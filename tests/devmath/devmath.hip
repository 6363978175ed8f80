// devmath.hip — test-only probe of the device branches of mdrp_math.h (tests/test_gpu_devmath.py).
//
// mdrp_math.h has a __HIP_DEVICE_COMPILE__ branch in its numeric primitives (hardware reciprocal / rsqrt seeds with Newton steps, the
// LDS-table log1p of the Cauchy losses, the FAST cubic, the rsqrt Cholesky); tests/hostmath compiles the header with g++ and so only ever
// sees the host branch.  This file exposes each device primitive as an element-wise kernel behind an extern "C" launcher that takes host
// arrays, so the test can compare it with an mpmath reference.  It is compiled by the test with the library's own flags
// (mdrp_amd/build.py FLAGS: -O3 -ffp-contract=fast) and is not part of the library.
#include <hip/hip_runtime.h>

#include "../../mdrp_amd/csrc/mdrp_math.h"
#include "../../mdrp_amd/csrc/mdrp_logtab.h"

namespace {

using namespace mdrp;

__device__ const double g_tab[MDRP_LOGTAB_N][2] = MDRP_LOGTAB_INIT;

enum { OP_SV_RCP, OP_SV_DIV, OP_SV_RSQRT, OP_SV_SQRT, OP_LM_RCP, OP_LM_RSQRT, OP_LM_LOG1P, OP_LOSS3, OP_LOSS4 };

constexpr int BLOCK = 256;

__global__ void __launch_bounds__(BLOCK) k_unary(int op, const double *a, const double *b, double *out, int n) {
    __shared__ double tab[2 * MDRP_LOGTAB_N];
    for (int i = threadIdx.x; i < 2 * MDRP_LOGTAB_N; i += blockDim.x) tab[i] = g_tab[i >> 1][i & 1];
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = a[i], y = b[i];
    double r;
    switch (op) {
    case OP_SV_RCP: r = sv_rcp(x); break;
    case OP_SV_DIV: r = sv_div(x, y); break;
    case OP_SV_RSQRT: r = sv_rsqrt(x); break;
    case OP_SV_SQRT: r = sv_sqrt(x); break;
    case OP_LM_RCP: r = lm_rcp(x); break;
    case OP_LM_RSQRT: r = lm_rsqrt(x); break;
    case OP_LM_LOG1P: r = lm_log1p(x, tab); break;
    case OP_LOSS3: r = loss_value_tab(3, x, y, tab); break; // (thr, r2)
    case OP_LOSS4: r = loss_value_tab(4, x, y, tab); break;
    default: r = __builtin_nan(""); break;
    }
    out[i] = r;
}

// coef: n x 3 (b, c, d) -> out: n x 4 (r0, r1, r2, number of real roots)
template <bool FAST>
__global__ void __launch_bounds__(BLOCK) k_cubic(const double *coef, double *out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double r0, r1, r2;
    const int nr = solve_cubic_real<FAST>(coef[3 * i], coef[3 * i + 1], coef[3 * i + 2], r0, r1, r2);
    out[4 * i] = r0; out[4 * i + 1] = r1; out[4 * i + 2] = r2; out[4 * i + 3] = (double)nr;
}

// coef: n x 4 (b, c, d, e) -> out: n x 5 (roots[0..3], validity mask)
__global__ void __launch_bounds__(BLOCK) k_quartic(const double *coef, double *out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double r[4];
    const int mask = solve_quartic_real(coef[4 * i], coef[4 * i + 1], coef[4 * i + 2], coef[4 * i + 3], r);
    out[5 * i] = r[0]; out[5 * i + 1] = r[1]; out[5 * i + 2] = r[2]; out[5 * i + 3] = r[3]; out[5 * i + 4] = (double)mask;
}

// A: n x N x N (row-major; chol_solve reads the lower triangle), b: n x N -> x: n x N
template <int N>
__global__ void __launch_bounds__(BLOCK) k_chol(const double *A, const double *b, double *x, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double a[N * N], v[N], s[N];
#pragma unroll
    for (int k = 0; k < N * N; ++k) a[k] = A[(size_t)i * N * N + k];
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = b[(size_t)i * N + k];
    chol_solve<N>(a, v, s);
#pragma unroll
    for (int k = 0; k < N; ++k) x[(size_t)i * N + k] = s[k];
}

// device buffers of one launcher call: put() copies an input in, finish() syncs and copies the result out; 0 or the first HIP error
struct Dev {
    double *p[3] = {nullptr, nullptr, nullptr};
    hipError_t err = hipSuccess;
    ~Dev() {
        for (double *q : p)
            if (q) (void)hipFree(q);
    }
    double *put(int k, const double *host, size_t count) {
        if (err != hipSuccess) return nullptr;
        err = hipMalloc(&p[k], count * sizeof(double) + 8);
        if (err == hipSuccess && host) err = hipMemcpy(p[k], host, count * sizeof(double), hipMemcpyHostToDevice);
        return p[k];
    }
    int finish(double *host_out, const double *dev_out, size_t count) {
        if (err == hipSuccess) err = hipGetLastError();
        if (err == hipSuccess) err = hipDeviceSynchronize();
        if (err == hipSuccess) err = hipMemcpy(host_out, dev_out, count * sizeof(double), hipMemcpyDeviceToHost);
        return (int)err;
    }
};

int grid(int n) { return (n + BLOCK - 1) / BLOCK; }

} // namespace

extern "C" {

// op: see the enum above; b is the second operand of sv_div and the r2 of the two losses (a is their thr); may be null otherwise
int dm_unary(int op, const double *a, const double *b, double *out, int n) {
    if (n <= 0) return 0;
    Dev d;
    const double *da = d.put(0, a, n), *db = d.put(1, b ? b : a, n);
    double *dout = d.put(2, nullptr, n);
    if (d.err == hipSuccess) hipLaunchKernelGGL(k_unary, dim3(grid(n)), dim3(BLOCK), 0, 0, op, da, db, dout, n);
    return d.finish(out, dout, n);
}

int dm_cubic(int fast, const double *coef, double *out, int n) {
    if (n <= 0) return 0;
    Dev d;
    const double *dc = d.put(0, coef, 3 * (size_t)n);
    double *dout = d.put(1, nullptr, 4 * (size_t)n);
    if (d.err == hipSuccess) {
        if (fast) hipLaunchKernelGGL(k_cubic<true>, dim3(grid(n)), dim3(BLOCK), 0, 0, dc, dout, n);
        else hipLaunchKernelGGL(k_cubic<false>, dim3(grid(n)), dim3(BLOCK), 0, 0, dc, dout, n);
    }
    return d.finish(out, dout, 4 * (size_t)n);
}

int dm_quartic(const double *coef, double *out, int n) {
    if (n <= 0) return 0;
    Dev d;
    const double *dc = d.put(0, coef, 4 * (size_t)n);
    double *dout = d.put(1, nullptr, 5 * (size_t)n);
    if (d.err == hipSuccess) hipLaunchKernelGGL(k_quartic, dim3(grid(n)), dim3(BLOCK), 0, 0, dc, dout, n);
    return d.finish(out, dout, 5 * (size_t)n);
}

// N in 5..9 (the parameter counts of the LM problems); anything else: -1
int dm_chol(int N, const double *A, const double *b, double *x, int n) {
    if (N < 5 || N > 9) return -1;
    if (n <= 0) return 0;
    Dev d;
    const double *dA = d.put(0, A, (size_t)n * N * N), *db = d.put(1, b, (size_t)n * N);
    double *dx = d.put(2, nullptr, (size_t)n * N);
    if (d.err == hipSuccess) {
        switch (N) {
        case 5: hipLaunchKernelGGL(k_chol<5>, dim3(grid(n)), dim3(BLOCK), 0, 0, dA, db, dx, n); break;
        case 6: hipLaunchKernelGGL(k_chol<6>, dim3(grid(n)), dim3(BLOCK), 0, 0, dA, db, dx, n); break;
        case 7: hipLaunchKernelGGL(k_chol<7>, dim3(grid(n)), dim3(BLOCK), 0, 0, dA, db, dx, n); break;
        case 8: hipLaunchKernelGGL(k_chol<8>, dim3(grid(n)), dim3(BLOCK), 0, 0, dA, db, dx, n); break;
        default: hipLaunchKernelGGL(k_chol<9>, dim3(grid(n)), dim3(BLOCK), 0, 0, dA, db, dx, n); break;
        }
    }
    return d.finish(x, dx, (size_t)n * N);
}

// the host branch of the same header (IEEE division and square root, library acos / cos), on the CPU: the yardstick of the FAST cubic and of
// the quartic, which has no IEEE variant on the device
void dm_cubic_host(const double *coef, double *out, int n) {
    for (int i = 0; i < n; ++i) {
        double r0, r1, r2;
        const int nr = solve_cubic_real<false>(coef[3 * i], coef[3 * i + 1], coef[3 * i + 2], r0, r1, r2);
        out[4 * i] = r0; out[4 * i + 1] = r1; out[4 * i + 2] = r2; out[4 * i + 3] = (double)nr;
    }
}

void dm_quartic_host(const double *coef, double *out, int n) {
    for (int i = 0; i < n; ++i) {
        double r[4];
        const int mask = solve_quartic_real(coef[4 * i], coef[4 * i + 1], coef[4 * i + 2], coef[4 * i + 3], r);
        out[5 * i] = r[0]; out[5 * i + 1] = r[1]; out[5 * i + 2] = r[2]; out[5 * i + 3] = r[3]; out[5 * i + 4] = (double)mask;
    }
}

} // extern "C"
