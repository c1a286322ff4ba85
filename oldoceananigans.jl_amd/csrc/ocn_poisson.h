// ocn_poisson.h -- the single-GPU Poisson solvers (src/Solvers/): the launchers of the LDS line-FFT kernels, FFTBasedPoissonSolver and
// FourierTridiagonalPoissonSolver on rocFFT plans with their creation-time self-checks and the per-direction fallback. Host code, included
// by ocn_api.hip behind the pressure-correction entry points.
#pragma once

// line-FFT kernels (ocn_line_fft.h): lines per workgroup by line length, see strided_line_fft_kernel; the longest line they take: 1024
// points x 4 lines x 16 B = the 64 KB of LDS a workgroup may ask for
#ifndef OCN_LINE_MAX
#define OCN_LINE_MAX 1024
#endif
static inline int line_zl(const OcnOptions &o, int n) { return n >= 1024 ? 4 : (n >= 512 ? o.line_zl512 : 8); }
// the line kernels exist for 4 and for 8 lines per workgroup: `launch` receives the count as an integral_constant
template <class F>
static inline void with_line_count(int lines, F &&launch) {
    if (lines == 4) launch(std::integral_constant<int, 4>{});
    else            launch(std::integral_constant<int, 8>{});
}
// ... and for these line lengths at compile time (1, 2, 4, 8 or 16 points per thread: all of a thread's loads in flight at once, see LineFFT);
// every other length -- fewer points than the 256 / lines k-rows of a pass -- takes the generic loops: `launch` receives (lines, length or 0)
template <class F>
static inline void with_line_shape(int lines, int n, F &&launch) {
    using std::integral_constant;
#if OCN_LINE_IN_FLIGHT
    if (lines == 4) {
        if (n == 512)  return launch(integral_constant<int, 4>{}, integral_constant<int, 512>{});
        if (n == 1024) return launch(integral_constant<int, 4>{}, integral_constant<int, 1024>{});
    } else {
        if (n == 32)  return launch(integral_constant<int, 8>{}, integral_constant<int, 32>{});
        if (n == 64)  return launch(integral_constant<int, 8>{}, integral_constant<int, 64>{});
        if (n == 128) return launch(integral_constant<int, 8>{}, integral_constant<int, 128>{});
        if (n == 256) return launch(integral_constant<int, 8>{}, integral_constant<int, 256>{});
        if (n == 512) return launch(integral_constant<int, 8>{}, integral_constant<int, 512>{});
    }
#endif
    with_line_count(lines, [&](auto ZL) { launch(ZL, integral_constant<int, 0>{}); });
}
static inline void launch_strided_line_fft(const OcnOptions &o, double2 *data, const double2 *tw, long C, long ncols, unsigned batches, int N, int logn, int inverse,
                                           double scale, long plane_stride = 0) {
    const int zl = line_zl(o, N);
    const dim3 grd((unsigned)((ncols + zl - 1) / zl), batches);
    const size_t lds = (size_t)N * zl * sizeof(double2);
    with_line_shape(zl, N, [&](auto ZL, auto NC) {
        hipLaunchKernelGGL((strided_line_fft_kernel<decltype(ZL)::value, decltype(NC)::value>), grd, dim3(256), lds, g_stream, data, tw, C, N, logn, inverse, scale, plane_stride);
    });
}
static inline void launch_paired_zline(const OcnOptions &o, bool forward, const double2 *in, double2 *out, const double2 *tw, long C, int N, int logn, double scale) {
    const int zl = line_zl(o, N);
    const dim3 grd((unsigned)((C + zl - 1) / zl));
    const size_t lds = (size_t)N * zl * sizeof(double2);
    if (forward) with_line_count(zl, [&](auto ZL) {
        hipLaunchKernelGGL(paired_zline_r2c_kernel<decltype(ZL)::value>, grd, dim3(256), lds, g_stream, in, out, tw, C, N, logn);
    });
    else with_line_count(zl, [&](auto ZL) {
        hipLaunchKernelGGL(paired_zline_c2r_kernel<decltype(ZL)::value>, grd, dim3(256), lds, g_stream, in, out, tw, C, N, logn, scale);
    });
}
// short lines (thin slabs) take the grouped Thomas kernels: 4 elements per lane and N / 4 lanes per line -- 2, 4 or 8 lines per wave
static inline bool xline_grouped(const OcnOptions &o, int N) { return o.dist_xline_group && (N == 32 || N == 64 || N == 128); }
template <bool SOLVE>
static inline void launch_xline_thomas(const OcnOptions &o, int E, double2 *S, const double *rden, long M, int N, double a, double2 *payload, const double2 *iface, double scale) {
    const dim3 blk(256);
    if (xline_grouped(o, N)) {
        const int lpw = 256 / N;
        const dim3 grp((unsigned)((M + 4 * lpw - 1) / (4 * lpw)));
        if (N == 32)       hipLaunchKernelGGL((xline_thomas_kernel<4, SOLVE, 8>), grp, blk, 0, g_stream, S, rden, M, N, a, payload, iface, scale);
        else if (N == 64)  hipLaunchKernelGGL((xline_thomas_kernel<4, SOLVE, 16>), grp, blk, 0, g_stream, S, rden, M, N, a, payload, iface, scale);
        else               hipLaunchKernelGGL((xline_thomas_kernel<4, SOLVE, 32>), grp, blk, 0, g_stream, S, rden, M, N, a, payload, iface, scale);
        return;
    }
    const dim3 grd((unsigned)((M + 3) / 4));
    switch (E) {
        case 1: hipLaunchKernelGGL((xline_thomas_kernel<1, SOLVE>), grd, blk, 0, g_stream, S, rden, M, N, a, payload, iface, scale); break;
        case 2: hipLaunchKernelGGL((xline_thomas_kernel<2, SOLVE>), grd, blk, 0, g_stream, S, rden, M, N, a, payload, iface, scale); break;
        case 4: hipLaunchKernelGGL((xline_thomas_kernel<4, SOLVE>), grd, blk, 0, g_stream, S, rden, M, N, a, payload, iface, scale); break;
        case 8: hipLaunchKernelGGL((xline_thomas_kernel<8, SOLVE>), grd, blk, 0, g_stream, S, rden, M, N, a, payload, iface, scale); break;
        default: hipLaunchKernelGGL((xline_thomas_kernel<16, SOLVE>), grd, blk, 0, g_stream, S, rden, M, N, a, payload, iface, scale); break;
    }
}
static inline void launch_zline_solve(const OcnOptions &o, double2 *hc, const double2 *tw, const double *lx, const double *ly, const double *lz, int Nxs, int Ny, int Nz,
                                      int logn, double scale, int pitch = 0) {
    const int zl = line_zl(o, Nz);
    const dim3 grd((unsigned)((Nxs + zl - 1) / zl), (unsigned)Ny);
    const size_t lds = (size_t)Nz * zl * sizeof(double2);
    with_line_shape(zl, Nz, [&](auto ZL, auto NC) {
        hipLaunchKernelGGL((zline_solve_kernel<decltype(ZL)::value, decltype(NC)::value>), grd, dim3(256), lds, g_stream, hc, tw, lx, ly, lz, Nxs, Ny, Nz, logn, scale, pitch);
    });
}

// ---- builders shared by both solvers' create functions ----
// a line the LDS line-FFT kernels take: a power of two from 8 to `max` points
static inline bool line_length_ok(int n, int max = OCN_LINE_MAX) { return n >= 8 && n <= max && (n & (n - 1)) == 0; }
static inline int ilog2(int n) {
    int logn = 0;
    while ((1 << logn) < n) ++logn;
    return logn;
}
// exp(-2πi m / n), m < n/2, on the device
static int upload_twiddles(int n, double2 **dst) {
    std::vector<double2> tw(n / 2);
    for (int m = 0; m < n / 2; ++m) {
        const double a = -2.0 * M_PI * (double)m / (double)n;
        tw[m] = make_double2(cos(a), sin(a));
    }
    HIP_TRY(dev_alloc((void **)dst, tw.size() * sizeof(double2)));
    HIP_TRY(hipMemcpy(*dst, tw.data(), tw.size() * sizeof(double2), hipMemcpyHostToDevice));
    return OCN_OK;
}
// a device temporary of a create function or a self-check: freed when its scope ends, whichever way that is
template <class T>
struct DevTmp {
    T *p = nullptr;
    DevTmp() = default;
    DevTmp(const DevTmp &) = delete;
    DevTmp &operator=(const DevTmp &) = delete;
    ~DevTmp() { hipFree(p); }
    hipError_t alloc(size_t count) { return dev_alloc((void **)&p, count * sizeof(T)); }
};
// the diagonal of the z-tridiagonal system of one horizontal mode (fourier_tridiagonal_poisson_solver.jl:180-210, HomogeneousZFormulation),
// host-built: Nz values `stride` apart; upload_tridiagonal_lower: the off-diagonal, the same for every mode.
// Nz == 1 (reachable for a stand-alone solver: Nz = Hz = 1 passes ocn_grid_create): the two assignments below hit the same entry and leave
// -1/dzf(1) - dzc(1) lxy, the serial solver's value; the distributed solver writes -dzc(1) lxy without calling this. Each keeps its value.
static void tridiagonal_column(ocn_grid_t grid, double lxy, double *col, size_t stride) {
    const int Nz = grid->d.Nz, Hz = grid->d.Hz;
    auto dzf = [&](int k) { return grid->h_dzf[k - 1 + Hz]; };
    auto dzc = [&](int k) { return grid->h_dzc[k - 1 + Hz]; };
    auto at = [&](int k) -> double & { return col[stride * (size_t)(k - 1)]; };
    at(1) = -1.0 / dzf(2) - dzc(1) * lxy;
    at(Nz) = -1.0 / dzf(Nz) - dzc(Nz) * lxy;
    for (int k = 2; k <= Nz - 1; ++k) at(k) = -(1.0 / dzf(k + 1) + 1.0 / dzf(k)) - dzc(k) * lxy;
}
static int upload_tridiagonal_lower(ocn_grid_t grid, double **dst) {
    const int Nz = grid->d.Nz, Hz = grid->d.Hz;
    std::vector<double> lower(std::max(1, Nz - 1));
    for (int q = 1; q <= Nz - 1; ++q) lower[q - 1] = 1.0 / grid->h_dzf[q + Hz];
    HIP_TRY(dev_alloc((void **)dst, lower.size() * sizeof(double)));
    HIP_TRY(hipMemcpy(*dst, lower.data(), lower.size() * sizeof(double), hipMemcpyHostToDevice));
    return OCN_OK;
}

struct ocn_poisson_s {
    ocn_grid_t grid;
    const OcnOptions *opt = nullptr;        // the owning model's options (standalone solvers: the library defaults)
    int kind;
    size_t n;                   // Nx*Ny*Nz
    double2 *storage = nullptr; // kind 0: rhs + solution; kind 1: solution
    double2 *source = nullptr;  // kind 1: rhs
    double *lam[3] = {nullptr, nullptr, nullptr};
    double *D = nullptr, *lower = nullptr, *t = nullptr;
    double2 *partial = nullptr, *mean = nullptr;
    hipfftHandle plan = 0;
    bool has_plan = false;
    // real-transform fast path used by solve_for_pressure! (the source term is real by construction): D2Z of a dense real
    // rhs into the Hermitian half spectrum (Nx/2+1, Ny, Nz), Z2D straight into the interior of the haloed pressure field
    int Nxh = 0;
    size_t nh = 0;
    double *rrhs = nullptr;      // dense real right-hand side / fallback real output
    double2 *hc = nullptr;       // half spectrum
    double2 *hc2 = nullptr;      // kind 1: tridiagonal solution (separate from the rhs like the reference's storage)
    hipfftHandle plan_r2c = 0, plan_c2r = 0;
    bool has_r2c = false, has_c2r = false, c2r_strided = false;
    bool zfused = false;         // kind 0: 2-D (x, y) plans + zline_solve_kernel instead of 3-D plans + divide kernel
    // split form of the 2-D (x, y) transforms for the model's time-step (Ny = 2^m <= 1024): 1-D R2C / C2R plans along x and the y
    // pass by strided_line_fft_kernel (61 us against the 82 us of the 2-D plan's column kernel); the inverse lands in the dense
    // real array, which the dense pressure correction (ocn_pressure_step.h) reads directly
    bool split = false;
    int Nxp = 0;                 // row pitch (complex elements) of hc / hc2 on the split path: Nxh rounded up to a multiple of 8
    hipfftHandle plan_xr2c = 0, plan_xc2r = 0;
    int logn_y = 0;
    double2 *ytw = nullptr;
    int logn_z = 0;
    double2 *ztw = nullptr;      // exp(-2πi m / Nz), m < Nz/2
    // grids with Bounded transformed directions: per-direction line transforms (see ocn_kernels.h, line_gather_kernel)
    bool general = false;
    hipfftHandle plan_line[3] = {0, 0, 0};
    bool has_line[3] = {false, false, false};   // owns the handle (directions of equal length share one plan)
    double2 *buffer = nullptr;
};

// Solvers/poisson_eigenvalues.jl:8-23
static void poisson_eigenvalues(int N, double L, int topo, std::vector<double> &lam) {
    lam.resize(N);
    if (topo == OCN_FLAT) { for (double &x : lam) x = 0.0; return; }      // poisson_eigenvalues(N, L, dim, ::Flat) = zeros
    for (int i = 1; i <= N; ++i) {
        double arg = topo == OCN_PERIODIC ? ((double)(i - 1) * M_PI) / (double)N : ((double)(i - 1) * M_PI) / (double)(2 * N);
        double s = 2.0 * sin(arg) / (L / (double)N);
        lam[i - 1] = s * s;
    }
}

extern "C" int ocn_poisson_destroy(ocn_poisson_t s) {
    if (!s) return OCN_OK;
    if (s->has_plan) hipfftDestroy(s->plan);
    if (s->split) { hipfftDestroy(s->plan_xr2c); hipfftDestroy(s->plan_xc2r); }
    hipFree(s->ytw);
    if (s->has_r2c) hipfftDestroy(s->plan_r2c);
    if (s->has_c2r) hipfftDestroy(s->plan_c2r);
    for (int d = 0; d < 3; ++d)
        if (s->has_line[d]) hipfftDestroy(s->plan_line[d]);
    hipFree(s->buffer);
    hipFree(s->ztw);
    hipFree(s->rrhs); hipFree(s->hc); hipFree(s->hc2);
    hipFree(s->storage); hipFree(s->source); hipFree(s->D); hipFree(s->lower); hipFree(s->t);
    hipFree(s->partial); hipFree(s->mean);
    for (int d = 0; d < 3; ++d) hipFree(s->lam[d]);
    delete s;
    return OCN_OK;
}

// ---- FFT plan self-checks -------------------------------------------------------------------------------------------
// rocFFT (7.0 and 7.2 tested) can return WRONG transforms from a freshly created plan while plans of other sizes are alive
// in the process (tools/fft_real_test2.hip reproduces it without this library: e.g. a 64x16x8 real 3-D plan created while
// 32^3 / 16^3 plans exist). Every plan set is therefore verified once, at creation, by a round trip on a pseudo-random
// pattern; a solver whose plans fail the check is refused (OCN_EFFT) instead of silently producing wrong pressure.
static int reduce_blockmax(double *d_blockmax, int nb, double *out) {
    std::vector<double> h(nb);
    HIP_TRY(hipMemcpyAsync(h.data(), d_blockmax, nb * sizeof(double), hipMemcpyDeviceToHost, g_stream));
    HIP_TRY(hipStreamSynchronize(g_stream));
    double m = 0;
    for (double x : h) m = (x > m || x != x) ? x : m;
    *out = m;
    return OCN_OK;
}

static int verify_real_plans(ocn_poisson_s *s) {
    const DGrid &g = s->grid->d;
    const int Px = g.Nx + 2 * g.Hx, Py = g.Ny + 2 * g.Hy, Pz = g.Nz + 2 * g.Hz;
    const long n = (long)s->n;
    const int nb = 256;
    DevTmp<double> tmp, bm;
    HIP_TRY(bm.alloc(nb));
    hipLaunchKernelGGL(selfcheck_fill_real, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, g_stream, s->rrhs, n);
    hipfftResult r = hipfftExecD2Z(s->plan_r2c, s->rrhs, (hipfftDoubleComplex *)s->hc);
    const double scale = (s->kind == 0 && !s->zfused) ? 1.0 / ((double)g.Nx * g.Ny * g.Nz) : 1.0 / ((double)g.Nx * g.Ny);
    if (r == HIPFFT_SUCCESS) {
        if (s->c2r_strided) {
            hipError_t e = tmp.alloc((size_t)Px * Py * Pz);
            if (e != hipSuccess) return fail((int)e, "self-check allocation: %s", hipGetErrorString(e));
            r = hipfftExecZ2D(s->plan_c2r, (hipfftDoubleComplex *)s->hc, tmp.p + g.Hx + (size_t)Px * (g.Hy + (size_t)Py * g.Hz));
            hipLaunchKernelGGL(selfcheck_compare_real, dim3(nb), dim3(256), 0, g_stream, tmp.p, g.Nx, g.Ny, g.Nz, Px, Py, g.Hx, g.Hy, g.Hz, scale, bm.p);
        } else {
            r = hipfftExecZ2D(s->plan_c2r, (hipfftDoubleComplex *)s->hc, s->rrhs);
            hipLaunchKernelGGL(selfcheck_compare_real, dim3(nb), dim3(256), 0, g_stream, s->rrhs, g.Nx, g.Ny, g.Nz, g.Nx, g.Ny, 0, 0, 0, scale, bm.p);
        }
    }
    double err = 0;
    int rc = r == HIPFFT_SUCCESS ? reduce_blockmax(bm.p, nb, &err) : fail(1000 + (int)r, "hipFFT exec failed in the plan self-check (%d)", (int)r);
    if (rc) return rc;
    if (!(err < 1e-10))
        return fail(OCN_EFFT, "rocFFT self-check failed for the %dx%dx%d real transform pair (round-trip error %.3g): rocFFT returns wrong "
                              "results from this plan while plans of other sizes are alive in the process; destroy the other "
                              "models/solvers first", g.Nx, g.Ny, g.Nz, err);
    return OCN_OK;
}

static int verify_complex_plan(hipfftHandle plan, double2 *buf, long n, double scale, const char *what) {
    const int nb = 256;
    DevTmp<double> bm;
    HIP_TRY(bm.alloc(nb));
    hipLaunchKernelGGL(selfcheck_fill_complex, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, g_stream, buf, n);
    hipfftResult r = hipfftExecZ2Z(plan, (hipfftDoubleComplex *)buf, (hipfftDoubleComplex *)buf, HIPFFT_FORWARD);
    if (r == HIPFFT_SUCCESS) r = hipfftExecZ2Z(plan, (hipfftDoubleComplex *)buf, (hipfftDoubleComplex *)buf, HIPFFT_BACKWARD);
    hipLaunchKernelGGL(selfcheck_compare_complex, dim3(nb), dim3(256), 0, g_stream, buf, n, scale, bm.p);
    double err = 0;
    int rc = r == HIPFFT_SUCCESS ? reduce_blockmax(bm.p, nb, &err) : fail(1000 + (int)r, "hipFFT exec failed in the plan self-check (%d)", (int)r);
    if (rc) return rc;
    if (!(err < 1e-10))
        return fail(OCN_EFFT, "rocFFT self-check failed for the %s plan (round-trip error %.3g): rocFFT returns wrong results from this "
                              "plan while plans of other sizes are alive in the process; destroy the other models/solvers first", what, err);
    HIP_TRY(hipMemsetAsync(buf, 0, n * sizeof(double2), g_stream));
    return OCN_OK;
}

// the LDS line kernel (strided_line_fft_kernel on N-point lines, C columns) is accepted only if it reproduces the rocFFT plan on
// pseudo-random data in `buf` (n complex elements), in both directions
static int line_fft_matches_plan(const OcnOptions &opt, hipfftHandle plan, double2 *buf, size_t n, const double2 *tw, long C, int N, int logn, bool *matches) {
    DevTmp<double2> ref;
    DevTmp<double> bm;
    HIP_TRY(ref.alloc(n));
    HIP_TRY(bm.alloc(256));
    double err[2] = {-1.0, -1.0};
    bool ok = true;
    for (int dir = 0; dir < 2 && ok; ++dir) {
        hipLaunchKernelGGL(selfcheck_fill_complex, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, g_stream, buf, (long)n);
        ok = hipMemcpyAsync(ref.p, buf, n * sizeof(double2), hipMemcpyDeviceToDevice, g_stream) == hipSuccess &&
             hipfftExecZ2Z(plan, (hipfftDoubleComplex *)ref.p, (hipfftDoubleComplex *)ref.p, dir ? HIPFFT_BACKWARD : HIPFFT_FORWARD) == HIPFFT_SUCCESS;
        launch_strided_line_fft(opt, buf, tw, C, C, 1, N, logn, dir, 1.0);
        hipLaunchKernelGGL(max_abs_diff_kernel, dim3(256), dim3(256), 0, g_stream, (const double *)ref.p, (const double *)buf, 2 * (long)n, bm.p);
        ok = ok && reduce_blockmax(bm.p, 256, &err[dir]) == OCN_OK;
    }
    *matches = ok && err[0] >= 0 && err[1] >= 0 && err[0] < 1e-10 * N && err[1] < 1e-10 * N;
    (void)hipGetLastError();
    return OCN_OK;
}

// FFT plans capture a stream at creation; re-point them when the library stream changed (ocn_set_stream)
static int plan_set_stream(hipfftHandle plan) {
    FFT_TRY(hipfftSetStream(plan, g_stream));
    return OCN_OK;
}

// complex-to-complex resources of the reference's API (solve!(ϕ, solver, b) with a complex b): created on first use so
// that the model fast path keeps only its two real plans alive
// rocFFT hazard (tools/fft_real_test2.hip): a multi-dimensional plan created while plans of OTHER sizes are alive in
// the process can return wrong transforms (e.g. the 64x16x8 real 3-D pair after 32x16x8, 8x16x32 and 32^3; exact again once the older
// plans are destroyed -- an internal cache of rocFFT keyed too coarsely). Triage on MI355X: the embedded (strided) Z2D plans and the
// unit-stride batched 1-D complex plans stay exact in exactly that situation. A solver whose multi-dimensional plans fail their
// creation-time self-check therefore switches to the per-direction path (gather -> unit-stride batched 1-D Z2Z -> scatter, the path
// of the cosine-transform topologies), which is verified in turn; only if that fails too is the solver refused (OCN_EFFT).
static int g_fft_fallbacks = 0;
static int ensure_complex(ocn_poisson_s *s);
static int poisson_fall_back(ocn_poisson_s *s) {
    (void)hipGetLastError();
    s->general = true;
    s->split = false;
    ++g_fft_fallbacks;
    return ensure_complex(s);
}
extern "C" int ocn_debug_fft_fallbacks(void) { return g_fft_fallbacks; }

static int ensure_complex(ocn_poisson_s *s) {
    if (s->has_plan || s->buffer) return OCN_OK;
    const DGrid &g = s->grid->d;
    if (!s->storage) HIP_TRY(dev_alloc((void **)&s->storage, s->n * sizeof(double2)));
    HIP_TRY(hipMemsetAsync(s->storage, 0, s->n * sizeof(double2), g_stream));
    if (s->kind == 1 && !s->source) {
        HIP_TRY(dev_alloc((void **)&s->source, s->n * sizeof(double2)));
        HIP_TRY(hipMemsetAsync(s->source, 0, s->n * sizeof(double2), g_stream));
        HIP_TRY(dev_alloc((void **)&s->partial, 1024 * sizeof(double2)));
        HIP_TRY(dev_alloc((void **)&s->mean, sizeof(double2)));
    }
    if (s->general) {
        HIP_TRY(dev_alloc((void **)&s->buffer, s->n * sizeof(double2)));
        const int N[3] = {g.Nx, g.Ny, g.Nz};
        const int ndims = s->kind == 0 ? 3 : 2;
        const int T[3] = {g.tx, g.ty, g.tz};
        for (int d = 0; d < ndims; ++d) {
            if (T[d] == OCN_FLAT) continue;
            int shared = -1;
            for (int e = 0; e < d; ++e)
                if (N[e] == N[d] && T[e] != OCN_FLAT) shared = e;
            if (shared >= 0) { s->plan_line[d] = s->plan_line[shared]; continue; }
            int nn[1] = {N[d]};
            hipfftResult r = hipfftPlanMany(&s->plan_line[d], 1, nn, nullptr, 1, N[d], nullptr, 1, N[d], HIPFFT_Z2Z, (int)(s->n / N[d]));
            if (r != HIPFFT_SUCCESS) return fail(1000 + (int)r, "hipfftPlanMany(line, dim %d) failed (%d)", d, (int)r);
            s->has_line[d] = true;
            FFT_TRY(hipfftSetStream(s->plan_line[d], g_stream));
            int rc = verify_complex_plan(s->plan_line[d], s->buffer, (long)s->n, 1.0 / (double)N[d], "line transform");
            if (rc) return rc;
        }
        return OCN_OK;
    }
    hipfftResult r;
    if (s->kind == 0) {
        r = hipfftPlan3d(&s->plan, g.Nz, g.Ny, g.Nx, HIPFFT_Z2Z);
    } else {
        int nfft[2] = {g.Ny, g.Nx};
        r = hipfftPlanMany(&s->plan, 2, nfft, nullptr, 1, g.Nx * g.Ny, nullptr, 1, g.Nx * g.Ny, HIPFFT_Z2Z, g.Nz);
    }
    if (r != HIPFFT_SUCCESS) return fail(1000 + (int)r, "hipfftPlan (Z2Z) failed (%d)", (int)r);
    s->has_plan = true;
    FFT_TRY(hipfftSetStream(s->plan, g_stream));
    const double scale = s->kind == 0 ? 1.0 / ((double)g.Nx * g.Ny * g.Nz) : 1.0 / ((double)g.Nx * g.Ny);
    int rc = verify_complex_plan(s->plan, s->storage, (long)s->n, scale, "complex-to-complex");
    if (rc != OCN_EFFT) return rc;
    // the multi-dimensional plan came out wrong (see poisson_fall_back): per-direction transforms on unit-stride 1-D plans instead
    hipfftDestroy(s->plan);
    s->has_plan = false;
    return poisson_fall_back(s);
}

// one direction of the transform on a grid with Bounded directions (forward: physical -> spectral)
static int transform_dim(ocn_poisson_s *s, double2 *A, int d, bool forward) {
    const DGrid &g = s->grid->d;
    const int T[3] = {g.tx, g.ty, g.tz};
    if (T[d] == OCN_FLAT) return OCN_OK;
    const int mode = T[d] == OCN_BOUNDED ? (forward ? 1 : 2) : 0;
    { int rc_ = plan_set_stream(s->plan_line[d]); if (rc_) return rc_; }
    const int dir = forward ? HIPFFT_FORWARD : HIPFFT_BACKWARD;
    if (mode == 0 && d == 0) {          // x lines are contiguous already
        FFT_TRY(hipfftExecZ2Z(s->plan_line[d], (hipfftDoubleComplex *)A, (hipfftDoubleComplex *)A, dir));
        return OCN_OK;
    }
    hipLaunchKernelGGL(line_gather_kernel, grid3(g.Nx, g.Ny, g.Nz, BLK), BLK, 0, g_stream, A, s->buffer, g.Nx, g.Ny, g.Nz, d, mode);
    FFT_TRY(hipfftExecZ2Z(s->plan_line[d], (hipfftDoubleComplex *)s->buffer, (hipfftDoubleComplex *)s->buffer, dir));
    hipLaunchKernelGGL(line_scatter_kernel, grid3(g.Nx, g.Ny, g.Nz, BLK), BLK, 0, g_stream, s->buffer, A, g.Nx, g.Ny, g.Nz, d, mode);
    KERNEL_CHECK();
    return OCN_OK;
}

// Bounded directions first on the way in, last on the way out (plan_transforms.jl:44-65)
static int transform_all(ocn_poisson_s *s, double2 *A, bool forward) {
    const DGrid &g = s->grid->d;
    const int T[3] = {g.tx, g.ty, g.tz};
    const int ndims = s->kind == 0 ? 3 : 2;
    for (int pass = 0; pass < 2; ++pass)
        for (int d = 0; d < ndims; ++d) {
            const bool bounded = T[d] == OCN_BOUNDED;
            if ((pass == 0) == (bounded == forward)) {
                int rc = transform_dim(s, A, d, forward);
                if (rc) return rc;
            }
        }
    return OCN_OK;
}

// fourier_tridiagonal_poisson_solver.jl:75-134: the tridiagonal data of kind 1
static int poisson_setup_tridiagonal(ocn_poisson_s *s, const std::vector<double> *lam) {
    const DGrid &g = s->grid->d;
    HIP_TRY(dev_alloc((void **)&s->D, s->n * sizeof(double)));
    HIP_TRY(dev_alloc((void **)&s->t, s->n * sizeof(double)));
    HIP_TRY(hipMemset(s->t, 0, s->n * sizeof(double)));
    { int rc_ = upload_tridiagonal_lower(s->grid, &s->lower); if (rc_) return rc_; }
    std::vector<double> D(s->n);
    for (int j = 0; j < g.Ny; ++j)
        for (int i = 0; i < g.Nx; ++i)
            tridiagonal_column(s->grid, lam[0][i] + lam[1][j], &D[(size_t)i + (size_t)g.Nx * j], (size_t)g.Nx * g.Ny);
    HIP_TRY(hipMemcpy(s->D, D.data(), s->n * sizeof(double), hipMemcpyHostToDevice));
    return OCN_OK;
}

// the buffers and the D2Z / Z2D plans of the real-transform path (the complex-to-complex resources of the reference API are created on
// first use)
static int poisson_setup_real_plans(ocn_poisson_s *s) {
    const DGrid &g = s->grid->d;
    const OcnOptions *opt = s->opt;
    const int kind = s->kind;
    s->Nxh = g.Nx / 2 + 1;
    s->nh = (size_t)s->Nxh * g.Ny * g.Nz;
    s->Nxp = (s->Nxh + 7) & ~7;                          // row pitch of the split path: whole 128-B rows
    const size_t nh_alloc = (size_t)s->Nxp * g.Ny * g.Nz;
    HIP_TRY(dev_alloc((void **)&s->rrhs, s->n * sizeof(double)));
    HIP_TRY(dev_alloc((void **)&s->hc, nh_alloc * sizeof(double2)));
    HIP_TRY(hipMemset(s->hc, 0, nh_alloc * sizeof(double2)));
    if (kind == 1) {
        HIP_TRY(dev_alloc((void **)&s->hc2, nh_alloc * sizeof(double2)));
        HIP_TRY(hipMemset(s->hc2, 0, nh_alloc * sizeof(double2)));
        HIP_TRY(hipMemset(s->hc2, 0, s->nh * sizeof(double2)));
    }
    const int Px = g.Nx + 2 * g.Hx, Py = g.Ny + 2 * g.Hy, Pz = g.Nz + 2 * g.Hz;
    if (kind == 0 && opt->fused_zfft && line_length_ok(g.Nz)) {
        s->zfused = true;
        s->logn_z = ilog2(g.Nz);
        { int rc_ = upload_twiddles(g.Nz, &s->ztw); if (rc_) return rc_; }
    }
    hipfftResult r;
    if (kind == 0 && !s->zfused) {
        int n3[3] = {g.Nz, g.Ny, g.Nx};
        r = hipfftPlanMany(&s->plan_r2c, 3, n3, nullptr, 1, 0, nullptr, 1, 0, HIPFFT_D2Z, 1);
        if (r != HIPFFT_SUCCESS) return fail(1000 + (int)r, "hipfftPlanMany(D2Z 3-D) failed (%d)", (int)r);
        s->has_r2c = true;
        int inembed[3] = {g.Nz, g.Ny, s->Nxh}, onembed[3] = {Pz, Py, Px};
        r = opt->c2r_strided ? hipfftPlanMany(&s->plan_c2r, 3, n3, inembed, 1, (int)s->nh, onembed, 1, Px * Py * Pz, HIPFFT_Z2D, 1) : HIPFFT_NOT_SUPPORTED;
        s->c2r_strided = r == HIPFFT_SUCCESS && opt->c2r_strided;
        if (!s->c2r_strided) r = hipfftPlanMany(&s->plan_c2r, 3, n3, nullptr, 1, 0, nullptr, 1, 0, HIPFFT_Z2D, 1);
        if (r != HIPFFT_SUCCESS) return fail(1000 + (int)r, "hipfftPlanMany(Z2D 3-D) failed (%d)", (int)r);
        s->has_c2r = true;
    } else {
        int n2[2] = {g.Ny, g.Nx};
        int rin[2] = {g.Ny, g.Nx}, cemb[2] = {g.Ny, s->Nxh}, pemb[2] = {Py, Px};
        r = hipfftPlanMany(&s->plan_r2c, 2, n2, rin, 1, g.Nx * g.Ny, cemb, 1, s->Nxh * g.Ny, HIPFFT_D2Z, g.Nz);
        if (r != HIPFFT_SUCCESS) return fail(1000 + (int)r, "hipfftPlanMany(D2Z 2-D) failed (%d)", (int)r);
        s->has_r2c = true;
        r = opt->c2r_strided ? hipfftPlanMany(&s->plan_c2r, 2, n2, cemb, 1, s->Nxh * g.Ny, pemb, 1, Px * Py, HIPFFT_Z2D, g.Nz) : HIPFFT_NOT_SUPPORTED;
        s->c2r_strided = r == HIPFFT_SUCCESS;
        if (!s->c2r_strided) r = hipfftPlanMany(&s->plan_c2r, 2, n2, cemb, 1, s->Nxh * g.Ny, rin, 1, g.Nx * g.Ny, HIPFFT_Z2D, g.Nz);
        if (r != HIPFFT_SUCCESS) return fail(1000 + (int)r, "hipfftPlanMany(Z2D 2-D) failed (%d)", (int)r);
        s->has_c2r = true;
    }
    if ((r = hipfftSetStream(s->plan_r2c, g_stream)) != HIPFFT_SUCCESS || (r = hipfftSetStream(s->plan_c2r, g_stream)) != HIPFFT_SUCCESS)
        return fail(1000 + (int)r, "hipfftSetStream failed (%d)", (int)r);
    return OCN_OK;
}

// the split form (1-D plans along x, y pass by strided_line_fft_kernel) is taken only if it passes: forward against the library's 2-D plan
// on pseudo-random data, inverse as a round trip of the split form. A failure of anything here leaves the 2-D plans in charge.
static void poisson_accept_split(ocn_poisson_s *s) {
    const DGrid &g = s->grid->d;
    int nx1[1] = {g.Nx};
    int rembx[1] = {g.Nx}, cembx[1] = {s->Nxp};
    hipfftResult r1 = hipfftPlanMany(&s->plan_xr2c, 1, nx1, rembx, 1, g.Nx, cembx, 1, s->Nxp, HIPFFT_D2Z, g.Ny * g.Nz);
    hipfftResult r2 = r1 == HIPFFT_SUCCESS ? hipfftPlanMany(&s->plan_xc2r, 1, nx1, cembx, 1, s->Nxp, rembx, 1, g.Nx, HIPFFT_Z2D, g.Ny * g.Nz) : r1;
    if (r1 == HIPFFT_SUCCESS && r2 != HIPFFT_SUCCESS) hipfftDestroy(s->plan_xr2c);
    if (r1 != HIPFFT_SUCCESS || r2 != HIPFFT_SUCCESS) return;
    hipfftSetStream(s->plan_xr2c, g_stream); hipfftSetStream(s->plan_xc2r, g_stream);
    s->logn_y = ilog2(g.Ny);
    DevTmp<double2> ref;
    DevTmp<double> bm;
    bool ok = upload_twiddles(g.Ny, &s->ytw) == OCN_OK && ref.alloc(s->nh) == hipSuccess && bm.alloc(256) == hipSuccess;
    double e_fwd = -1.0, e_rt = -1.0;
    if (ok) {
        const long n = (long)s->n;
        hipLaunchKernelGGL(selfcheck_fill_real, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, g_stream, s->rrhs, n);
        ok = hipfftExecD2Z(s->plan_r2c, s->rrhs, (hipfftDoubleComplex *)ref.p) == HIPFFT_SUCCESS &&
             hipfftExecD2Z(s->plan_xr2c, s->rrhs, (hipfftDoubleComplex *)s->hc) == HIPFFT_SUCCESS;
        launch_strided_line_fft(*s->opt, s->hc, s->ytw, (long)s->Nxp, (long)s->Nxp, (unsigned)g.Nz, g.Ny, s->logn_y, 0, 1.0, (long)s->Nxp * g.Ny);
        hipLaunchKernelGGL(max_abs_diff_pitched_kernel, dim3(256), dim3(256), 0, g_stream, (const double2 *)ref.p, s->Nxh,
                           (const double2 *)s->hc, s->Nxp, s->Nxh, (long)g.Ny * g.Nz, bm.p);
        ok = ok && reduce_blockmax(bm.p, 256, &e_fwd) == OCN_OK;
        launch_strided_line_fft(*s->opt, s->hc, s->ytw, (long)s->Nxp, (long)s->Nxp, (unsigned)g.Nz, g.Ny, s->logn_y, 1, 1.0, (long)s->Nxp * g.Ny);
        ok = ok && hipfftExecZ2D(s->plan_xc2r, (hipfftDoubleComplex *)s->hc, s->rrhs) == HIPFFT_SUCCESS;
        hipLaunchKernelGGL(selfcheck_compare_real, dim3(256), dim3(256), 0, g_stream, s->rrhs, g.Nx, g.Ny, g.Nz, g.Nx, g.Ny, 0, 0, 0,
                           1.0 / ((double)g.Nx * g.Ny), bm.p);
        ok = ok && reduce_blockmax(bm.p, 256, &e_rt) == OCN_OK;
    }
    s->split = ok && e_fwd >= 0 && e_fwd < 1e-10 * g.Nx * g.Ny && e_rt >= 0 && e_rt < 1e-10;
    if (!s->split) { hipfftDestroy(s->plan_xr2c); hipfftDestroy(s->plan_xc2r); }
    (void)hipGetLastError();
}

// everything a fresh solver owns; on an error the caller destroys the half-built solver
static int poisson_setup(ocn_poisson_s *s) {
    const DGrid &g = s->grid->d;
    const int kind = s->kind;
    const int N[3] = {g.Nx, g.Ny, g.Nz}, T[3] = {g.tx, g.ty, g.tz};
    std::vector<double> lam[3];
    for (int d = 0; d < 3; ++d) {
        poisson_eigenvalues(N[d], s->grid->L[d], T[d], lam[d]);
        HIP_TRY(dev_alloc((void **)&s->lam[d], N[d] * sizeof(double)));
        HIP_TRY(hipMemcpy(s->lam[d], lam[d].data(), N[d] * sizeof(double), hipMemcpyHostToDevice));
    }
    int rc;
    if (kind == 1 && (rc = poisson_setup_tridiagonal(s, lam))) return rc;
    if (s->general) return ensure_complex(s);      // cosine transforms: complex storage + per-direction line transforms, created (and verified) now
    if ((rc = poisson_setup_real_plans(s))) return rc;
    if ((rc = verify_real_plans(s))) {
        if (rc != OCN_EFFT) return rc;
        hipfftDestroy(s->plan_r2c); hipfftDestroy(s->plan_c2r);
        s->has_r2c = s->has_c2r = false;
        return poisson_fall_back(s);
    }
    if (s->opt->split_solve && (kind == 1 || s->zfused) && line_length_ok(g.Ny) && g.tx == OCN_PERIODIC && g.ty == OCN_PERIODIC) poisson_accept_split(s);
    return OCN_OK;
}

static int poisson_create(ocn_poisson_t *solver, ocn_grid_t grid, int kind, const OcnOptions *opt) {
    NEED_INIT();
    if (!solver || !grid) return fail(OCN_EINVAL, "NULL argument");
    const DGrid &g = grid->d;
    for (int t : {g.tx, g.ty, g.tz})
        if (t != OCN_PERIODIC && t != OCN_BOUNDED && t != OCN_FLAT)
            return fail(OCN_ENOTSUP, "Poisson solvers need Periodic or Bounded directions (a FullyConnected x belongs to ocn_dist_poisson_create)");
    if (kind == -1) kind = (g.tz == OCN_BOUNDED) ? 1 : 0;   // see DESIGN.md: z-Bounded takes the tridiagonal path by default
    if (kind == 0 && !grid->z_regular) return fail(OCN_EINVAL, "FFTBasedPoissonSolver requires a regular grid");
    if (kind == 1 && g.tz != OCN_BOUNDED)
        return fail(OCN_EINVAL, "`FourierTridiagonalPoissonSolver` can only be used when the stretched direction's topology is `Bounded`.");
    if (kind != 0 && kind != 1) return fail(OCN_EINVAL, "unknown solver kind %d", kind);
    ocn_poisson_s *s = new ocn_poisson_s();
    s->grid = grid; s->opt = opt; s->kind = kind;
    s->n = (size_t)g.Nx * g.Ny * g.Nz;
    s->general = g.tx == OCN_BOUNDED || g.ty == OCN_BOUNDED || (kind == 0 && g.tz == OCN_BOUNDED) ||
                 g.tx == OCN_FLAT || g.ty == OCN_FLAT || g.tz == OCN_FLAT;      // Flat directions are not transformed
    const int rc = poisson_setup(s);
    if (rc) { ocn_poisson_destroy(s); return rc; }
    *solver = s;
    return OCN_OK;
}
extern "C" int ocn_poisson_create(ocn_poisson_t *solver, ocn_grid_t grid, int kind) { return poisson_create(solver, grid, kind, &g_defaults); }

extern "C" int ocn_poisson_kind(ocn_poisson_t s) { return s ? s->kind : OCN_EINVAL; }

extern "C" int ocn_poisson_rhs(ocn_poisson_t s, double **rhs_complex) {
    if (!s || !rhs_complex) return fail(OCN_EINVAL, "NULL argument");
    NEED_INIT();
    { int rc_ = ensure_complex(s); if (rc_) return rc_; }
    *rhs_complex = (double *)(s->kind == 0 ? s->storage : s->source);
    return OCN_OK;
}

static int poisson_solve(ocn_poisson_s *s, double *phi) {
    const DGrid &g = s->grid->d;
    int rc;
    if ((rc = ensure_complex(s))) return rc;
    if (!s->general && (rc = plan_set_stream(s->plan))) return rc;
    // all transformed directions: the per-direction line transforms (Bounded directions, the fallback) or the one rocFFT plan
    auto transform = [&](double2 *A, bool forward) -> int {
        if (s->general) return transform_all(s, A, forward);
        FFT_TRY(hipfftExecZ2Z(s->plan, (hipfftDoubleComplex *)A, (hipfftDoubleComplex *)A, forward ? HIPFFT_FORWARD : HIPFFT_BACKWARD));
        return OCN_OK;
    };
    const double scale = s->kind == 0 ? 1.0 / ((double)g.Nx * (double)g.Ny * (double)g.Nz) : 1.0 / ((double)g.Nx * (double)g.Ny);
    const double2 *mean = nullptr;
    if (s->kind == 0) {
        // fft_based_poisson_solver.jl:95-125
        if ((rc = transform(s->storage, true))) return rc;
        hipLaunchKernelGGL(spectral_divide_kernel, grid3(g.Nx, g.Ny, g.Nz, BLK), BLK, 0, g_stream, s->storage, s->lam[0],
                           s->lam[1], s->lam[2], g.Nx, g.Ny, g.Nz, 1.0, false);
        if ((rc = transform(s->storage, false))) return rc;
    } else {
        // fourier_tridiagonal_poisson_solver.jl:212-239
        if ((rc = transform(s->source, true))) return rc;
        hipLaunchKernelGGL(tridiagonal_z_kernel, dim3((g.Nx + 63) / 64, g.Ny), dim3(64), 0, g_stream, g.Nx, g.Nx, g.Ny, g.Nz, s->lower,
                           s->D, s->lower, s->source, s->t, s->storage, 1.0, false);
        if ((rc = transform(s->storage, false))) return rc;
        const int nb = 1024;
        hipLaunchKernelGGL(sum_partial_kernel, dim3(nb), dim3(256), 0, g_stream, s->storage, (long)s->n, s->partial);
        hipLaunchKernelGGL(sum_final_kernel, dim3(1), dim3(256), 0, g_stream, s->partial, nb, 1.0 / (double)s->n, scale, s->mean);
        mean = s->mean;
        // the reference keeps the (normalised, mean-free) solution in `storage` between solves; the guarded update of the
        // singular column re-reads it (batched_tridiagonal_solver.jl:234-237). The read value only shifts the solution
        // by a constant that the mean removal deletes, so `storage` keeps the unnormalised field here.
    }
    hipLaunchKernelGGL(copy_real_kernel, grid3(g.Nx, g.Ny, g.Nz, BLK), BLK, 0, g_stream, g, make_view(g, phi, LOC_C), s->storage, scale, true, mean);
    KERNEL_CHECK();
    return OCN_OK;
}

// solve_for_pressure! on the real-transform path: rrhs (dense real, already filled by the source-term kernel) -> phi
static int poisson_solve_real(ocn_poisson_s *s, double *phi) {
    const DGrid &g = s->grid->d;
    const int Px = g.Nx + 2 * g.Hx, Py = g.Ny + 2 * g.Hy;
    double *interior = phi + g.Hx + (size_t)Px * (g.Hy + (size_t)Py * g.Hz);
    { int rc_; if ((rc_ = plan_set_stream(s->plan_r2c)) || (rc_ = plan_set_stream(s->plan_c2r))) return rc_; }
    FFT_TRY(hipfftExecD2Z(s->plan_r2c, s->rrhs, (hipfftDoubleComplex *)s->hc));
    double2 *sol = s->hc;
    if (s->kind == 0 && s->zfused) {
        const double scale = 1.0 / ((double)g.Nx * (double)g.Ny * (double)g.Nz);
        launch_zline_solve(*s->opt, s->hc, s->ztw, s->lam[0], s->lam[1], s->lam[2], s->Nxh, g.Ny, g.Nz, s->logn_z, scale);
    } else if (s->kind == 0) {
        const double scale = 1.0 / ((double)g.Nx * (double)g.Ny * (double)g.Nz);
        hipLaunchKernelGGL(spectral_divide_kernel, grid3(s->Nxh, g.Ny, g.Nz, BLK), BLK, 0, g_stream, s->hc, s->lam[0], s->lam[1],
                           s->lam[2], s->Nxh, g.Ny, g.Nz, scale, true);
    } else {
        const double scale = 1.0 / ((double)g.Nx * (double)g.Ny);
        hipLaunchKernelGGL(tridiagonal_z_kernel, dim3((s->Nxh + 63) / 64, g.Ny), dim3(64), 0, g_stream, s->Nxh, g.Nx, g.Ny, g.Nz,
                           s->lower, s->D, s->lower, s->hc, s->t, s->hc2, scale, true);
        hipLaunchKernelGGL(remove_mean_mode_kernel, dim3(1), dim3(256), 0, g_stream, s->hc2, (long)s->Nxh * g.Ny, g.Nz);
        sol = s->hc2;
    }
    if (s->c2r_strided) {
        FFT_TRY(hipfftExecZ2D(s->plan_c2r, (hipfftDoubleComplex *)sol, interior));
    } else {
        FFT_TRY(hipfftExecZ2D(s->plan_c2r, (hipfftDoubleComplex *)sol, s->rrhs));
        launch_copy_dense_to_field(g, phi, DenseSolution{s->rrhs, {}});        // (fallback when the strided C2R plan is unavailable)
    }
    KERNEL_CHECK();
    return OCN_OK;
}

// the same solve in split form: rrhs (dense real source term) -> rrhs (dense real solution, not yet divided by anything)
static int poisson_solve_real_split(ocn_poisson_s *s) {
    const DGrid &g = s->grid->d;
    { int rc_; if ((rc_ = plan_set_stream(s->plan_xr2c)) || (rc_ = plan_set_stream(s->plan_xc2r))) return rc_; }
    // rows of pitch Nxp: whole, 128-B aligned groups of lines
    FFT_TRY(hipfftExecD2Z(s->plan_xr2c, s->rrhs, (hipfftDoubleComplex *)s->hc));
    launch_strided_line_fft(*s->opt, s->hc, s->ytw, (long)s->Nxp, (long)s->Nxp, (unsigned)g.Nz, g.Ny, s->logn_y, 0, 1.0, (long)s->Nxp * g.Ny);
    double2 *sol = s->hc;
    if (s->kind == 0) {
        const double scale = 1.0 / ((double)g.Nx * (double)g.Ny * (double)g.Nz);
        launch_zline_solve(*s->opt, s->hc, s->ztw, s->lam[0], s->lam[1], s->lam[2], s->Nxh, g.Ny, g.Nz, s->logn_z, scale, s->Nxp);
    } else {
        const double scale = 1.0 / ((double)g.Nx * (double)g.Ny);
        hipLaunchKernelGGL(tridiagonal_z_kernel, dim3((s->Nxh + 63) / 64, g.Ny), dim3(64), 0, g_stream, s->Nxh, g.Nx, g.Ny, g.Nz,
                           s->lower, s->D, s->lower, s->hc, s->t, s->hc2, scale, true, s->Nxp);
        hipLaunchKernelGGL(remove_mean_mode_kernel, dim3(1), dim3(256), 0, g_stream, s->hc2, (long)s->Nxp * g.Ny, g.Nz);
        sol = s->hc2;
    }
    launch_strided_line_fft(*s->opt, sol, s->ytw, (long)s->Nxp, (long)s->Nxp, (unsigned)g.Nz, g.Ny, s->logn_y, 1, 1.0, (long)s->Nxp * g.Ny);
    FFT_TRY(hipfftExecZ2D(s->plan_xc2r, (hipfftDoubleComplex *)sol, s->rrhs));
    KERNEL_CHECK();
    return OCN_OK;
}

static int solve_for_pressure(ocn_poisson_s *s, const double *u, const double *v, const double *w, double *p) {
    const DGrid &g = s->grid->d;
    int rc;
    if (s->opt->real_fft && !s->general) {
        if ((rc = source_term(g, u, v, w, s->rrhs, s->kind == 1, true))) return rc;
        return poisson_solve_real(s, p);
    }
    if ((rc = ensure_complex(s))) return rc;
    if ((rc = source_term(g, u, v, w, s->kind == 0 ? s->storage : s->source, s->kind == 1))) return rc;
    return poisson_solve(s, p);
}

extern "C" int ocn_poisson_solve(ocn_poisson_t s, double *phi) {
    NEED_INIT();
    if (!s || !phi) return fail(OCN_EINVAL, "NULL argument");
    return poisson_solve(s, phi);
}

extern "C" int ocn_solve_for_pressure(ocn_poisson_t s, const double *u, const double *v, const double *w, double *p) {
    NEED_INIT();
    if (!s || !u || !v || !w || !p) return fail(OCN_EINVAL, "NULL argument");
    return solve_for_pressure(s, u, v, w, p);
}

extern "C" int ocn_batched_tridiagonal_solve_z(int Nx, int Ny, int Nz, const double *a, const double *b, const double *c,
                                               const double *f_complex, double *t, double *phi_complex) {
    NEED_INIT();
    if (Nx < 1 || Ny < 1 || Nz < 1 || !a || !b || !c || !f_complex || !t || !phi_complex) return fail(OCN_EINVAL, "invalid argument");
    if ((const void *)f_complex == (const void *)phi_complex || (const void *)t == (const void *)b)
        return fail(OCN_EINVAL, "the right-hand side and the solution (and the scratch and the diagonal) must be distinct arrays");
    hipLaunchKernelGGL(tridiagonal_z_kernel, dim3((Nx + 63) / 64, Ny), dim3(64), 0, g_stream, Nx, Nx, Ny, Nz, a, b, c,
                       (const double2 *)f_complex, t, (double2 *)phi_complex, 1.0, false);
    KERNEL_CHECK();
    return OCN_OK;
}
