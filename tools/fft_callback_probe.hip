// Probe: what does a rocFFT load callback cost on the x real-to-complex transform of the pressure solve?
//   hipcc --offload-arch=gfx950 -O3 -fgpu-rdc -ffp-contract=off tools/fft_callback_probe.hip -o tools/_bin/fft_callback_probe -lhipfft
//   tools/_bin/fft_callback_probe [N = 256]
// N^3 cells, triply periodic, dense u, v, w. Three ways to the half spectrum (rows of N reals -> N/2 + 1 complex at a padded pitch):
//   (a) the plain D2Z plan on a stored right-hand side;   (b) a divergence kernel that stores it, then (a);
//   (c) a D2Z plan whose load callback (hipfftXtSetCallback, HIPFFT_CB_LD_REAL_DOUBLE) forms the divergence from u, v, w on the fly.
// Prints the time of each (HIP events, mean of 20 after 3 warm-up calls) and whether (c) equals (b) bit for bit.
#include <hip/hip_runtime.h>
#include <hipfft/hipfft.h>
#include <hipfft/hipfftXt.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)
#define FFT(x) do { hipfftResult r_ = (x); if (r_ != HIPFFT_SUCCESS) { printf("%s: hipfft error %d\n", #x, (int)r_); return 3; } } while (0)

struct DivArgs { const double *u, *v, *w; int N; double ax, ay, az, vinv; };

__device__ __forceinline__ double divergence(const DivArgs &a, int i, int j, int k) {
    const int N = a.N, ip = i + 1 == N ? 0 : i + 1, jp = j + 1 == N ? 0 : j + 1, kp = k + 1 == N ? 0 : k + 1;
    const long row = (long)N * (j + (long)N * k);
    const double dx = a.ax * a.u[ip + row] - a.ax * a.u[i + row];
    const double dy = a.ay * a.v[i + (long)N * (jp + (long)N * k)] - a.ay * a.v[i + row];
    const double dz = a.az * a.w[i + (long)N * (j + (long)N * kp)] - a.az * a.w[i + row];
    return a.vinv * ((dx + dy) + dz);
}
__global__ void __launch_bounds__(256) divergence_kernel(DivArgs a, double *rhs) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y, k = blockIdx.z;
    if (i < a.N) rhs[i + (long)a.N * (j + (long)a.N * k)] = divergence(a, i, j, k);
}
__device__ double load_divergence(void *, size_t offset, void *info, void *) {
    const DivArgs a = *(const DivArgs *)info;
    const int i = (int)(offset % (size_t)a.N);
    const size_t r = offset / (size_t)a.N;
    const size_t k = r / (size_t)a.N;
    return divergence(a, i, (int)(r % (size_t)a.N), k < (size_t)a.N ? (int)k : a.N - 1);      // (no read outside the arrays, whatever offset arrives)
}
__device__ hipfftCallbackLoadD load_divergence_ptr = load_divergence;

int main(int argc, char **argv) {
    const int N = argc > 1 ? atoi(argv[1]) : 256;
    const size_t cells = (size_t)N * N * N;
    const int Nxh = N / 2 + 1, Nxp = (Nxh + 7) / 8 * 8;
    const size_t spec = (size_t)Nxp * N * N;
    std::vector<double> h(cells);
    double *u, *v, *w, *rhs;
    hipfftDoubleComplex *sb, *sc;
    DivArgs *dargs;
    CHECK(hipMalloc(&u, cells * 8)); CHECK(hipMalloc(&v, cells * 8)); CHECK(hipMalloc(&w, cells * 8)); CHECK(hipMalloc(&rhs, cells * 8));
    CHECK(hipMalloc(&sb, spec * 16)); CHECK(hipMalloc(&sc, spec * 16)); CHECK(hipMalloc(&dargs, sizeof(DivArgs)));
    CHECK(hipMemset(sb, 0, spec * 16)); CHECK(hipMemset(sc, 0, spec * 16));
    unsigned long long x = 88172645463325252ull;
    for (double *d : {u, v, w}) {
        for (size_t q = 0; q < cells; ++q) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; h[q] = (double)(x >> 11) / 9007199254740992.0 - 0.5; }
        CHECK(hipMemcpy(d, h.data(), cells * 8, hipMemcpyHostToDevice));
    }
    const DivArgs a{u, v, w, N, 0.25, 0.5, 0.125, 3.0};
    CHECK(hipMemcpy(dargs, &a, sizeof a, hipMemcpyHostToDevice));
    int n1[1] = {N}, rem[1] = {N}, cem[1] = {Nxp};
    hipfftHandle plain, cb;
    FFT(hipfftPlanMany(&plain, 1, n1, rem, 1, N, cem, 1, Nxp, HIPFFT_D2Z, N * N));
    FFT(hipfftPlanMany(&cb, 1, n1, rem, 1, N, cem, 1, Nxp, HIPFFT_D2Z, N * N));
    void *fn = nullptr, *info = dargs;
    CHECK(hipMemcpyFromSymbol(&fn, HIP_SYMBOL(load_divergence_ptr), sizeof fn));
    FFT(hipfftXtSetCallback(cb, &fn, HIPFFT_CB_LD_REAL_DOUBLE, &info));
    printf("callback set; N = %d, %d rows, spectrum pitch %d\n", N, N * N, Nxp); fflush(stdout);
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    const dim3 grd((N + 255) / 256, N, N);
    float ms[3] = {0, 0, 0};
    for (int which = 0; which < 3; ++which) {
        for (int rep = 0; rep < 23; ++rep) {
            if (rep == 3) CHECK(hipEventRecord(e0, 0));
            if (which == 1) hipLaunchKernelGGL(divergence_kernel, grd, dim3(256), 0, 0, a, rhs);
            if (which <= 1) FFT(hipfftExecD2Z(plain, rhs, sb));
            else FFT(hipfftExecD2Z(cb, u, sc));
        }
        CHECK(hipEventRecord(e1, 0));
        CHECK(hipEventSynchronize(e1));
        CHECK(hipGetLastError());
        CHECK(hipEventElapsedTime(&ms[which], e0, e1));
        printf("%s: %.1f us per call\n", which == 0 ? "(a) plain plan" : which == 1 ? "(b) divergence kernel + plain plan" : "(c) callback plan", 1e3 * ms[which] / 20);
        fflush(stdout);
    }
    std::vector<double> hb(2 * spec), hc(2 * spec);
    CHECK(hipMemcpy(hb.data(), sb, spec * 16, hipMemcpyDeviceToHost)); CHECK(hipMemcpy(hc.data(), sc, spec * 16, hipMemcpyDeviceToHost));
    size_t differing = 0;
    for (size_t row = 0; row < (size_t)N * N; ++row)
        for (int c = 0; c < 2 * Nxh; ++c) differing += memcmp(&hb[2 * row * Nxp + c], &hc[2 * row * Nxp + c], 8) != 0;
    printf("(c) against (b): %zu of %zu values differ\n", differing, (size_t)N * N * 2 * Nxh);
    return differing ? 1 : 0;
}
