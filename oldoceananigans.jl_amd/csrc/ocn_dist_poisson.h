// ocn_dist_poisson.h -- the distributed x-slab pieces (src/DistributedComputations): the x-halo pack / unpack entry points and the
// distributed Poisson solvers for Partition(R, 1, 1), every layout of ocn_dist_poisson_create and its step-time stages. The collectives
// themselves (RCCL send/recv, all-to-all) are issued by the host layer through torch.distributed on buffers it owns; the library packs /
// unpacks / transforms. Host code, included by ocn_api.hip behind ocn_poisson.h.
#pragma once

static int x_halo_buffers(const DGrid &g, double *const *fields, const int (*locs)[3], int n, double *west, double *east, bool pack,
                          int depth = 0) {
    // a wall side has no neighbour: nothing is unpacked there (what was packed for it is ignored by the other end of the ring)
    const bool do_west = pack || !wall_lo(g.tx), do_east = pack || !wall_hi(g.tx);
    if (n <= 0) return OCN_OK;
    if (depth <= 0) depth = g.Hx;
    if (depth > g.Hx || depth > g.Nx) return fail(OCN_EINVAL, "exchange depth %d exceeds the halo (%d) or the local interior (%d)", depth, g.Hx, g.Nx);
    if (n > OCN_MAX_FIELDS) return fail(OCN_EINVAL, "at most %d fields per call", OCN_MAX_FIELDS);
    FieldList fl;
    SlabList sl;
    fl.n = n;
    long off = 0, maxrows = 0;
    for (int f = 0; f < n; ++f) {
        int P[3];
        parent_size(g, locs[f], P);
        sl.p0[f] = P[0];                            // Face-in-x fields of a LeftConnected rank are one column longer
        fl.p[f] = fields[f];
        sl.off[f] = off;
        sl.rows[f] = (long)P[1] * P[2];
        off += (long)depth * sl.rows[f];
        maxrows = std::max(maxrows, sl.rows[f]);
    }
    const long threads = (long)depth * maxrows;
    const int nb = (int)((threads + 255) / 256);
    if (pack) hipLaunchKernelGGL(x_halo_buffer_kernel<true>, dim3(nb), dim3(256), 0, g_stream, fl, sl, g.Nx, g.Hx, depth, west, east, true, true);
    else      hipLaunchKernelGGL(x_halo_buffer_kernel<false>, dim3(nb), dim3(256), 0, g_stream, fl, sl, g.Nx, g.Hx, depth, west, east, do_west, do_east);
    KERNEL_CHECK();
    return OCN_OK;
}

extern "C" int ocn_pack_x_halos(ocn_grid_t grid, double *const *fields, const int (*locs)[3], int nfields, double *west_send,
                                double *east_send) {
    NEED_INIT();
    if (!grid || !fields || !locs || !west_send || !east_send) return fail(OCN_EINVAL, "NULL argument");
    return x_halo_buffers(grid->d, fields, locs, nfields, west_send, east_send, true);
}

extern "C" int ocn_unpack_x_halos(ocn_grid_t grid, double *const *fields, const int (*locs)[3], int nfields,
                                  const double *west_recv, const double *east_recv) {
    NEED_INIT();
    if (!grid || !fields || !locs || !west_recv || !east_recv) return fail(OCN_EINVAL, "NULL argument");
    return x_halo_buffers(grid->d, fields, locs, nfields, const_cast<double *>(west_recv), const_cast<double *>(east_recv), false);
}

extern "C" int ocn_pack_x_halos_depth(ocn_grid_t grid, double *const *fields, const int (*locs)[3], int nfields, int depth,
                                      double *west_send, double *east_send) {
    NEED_INIT();
    if (!grid || !fields || !locs || !west_send || !east_send) return fail(OCN_EINVAL, "NULL argument");
    if (depth < 1) return fail(OCN_EINVAL, "depth must be >= 1");
    return x_halo_buffers(grid->d, fields, locs, nfields, west_send, east_send, true, depth);
}

extern "C" int ocn_unpack_x_halos_depth(ocn_grid_t grid, double *const *fields, const int (*locs)[3], int nfields, int depth,
                                        const double *west_recv, const double *east_recv) {
    NEED_INIT();
    if (!grid || !fields || !locs || !west_recv || !east_recv) return fail(OCN_EINVAL, "NULL argument");
    if (depth < 1) return fail(OCN_EINVAL, "depth must be >= 1");
    return x_halo_buffers(grid->d, fields, locs, nfields, const_cast<double *>(west_recv), const_cast<double *>(east_recv), false, depth);
}

// DistributedFFTBasedPoissonSolver (distributed_fft_based_poisson_solver.jl:92-188) and
// DistributedFourierTridiagonalPoissonSolver (distributed_fft_tridiagonal_solver.jl:153-293) for Partition(R, 1, 1).
// z is never partitioned on an x-slab decomposition, so both solvers share one pipeline:
//   local complex transform in (y, z) [z Periodic] or y only [z Bounded] of the PAIRED real columns (see ocn_kernels.h)
//   -> separate + pack half the y modes -> all-to-all -> x transform -> spectral divide | z-tridiagonal solve
//   -> inverse x transform -> pack -> all-to-all -> rebuild full spectrum -> inverse local transform -> haloed pressure.
struct ocn_dist_poisson_s {
    ocn_grid_t grid;            // LOCAL grid (Nxl, Ny, Nz)
    const OcnOptions *opt = nullptr;        // the owning model's options (standalone solvers: the library defaults)
    int R, rank, zmode;         // zmode 0: z Periodic (FFT); 1: z Bounded (tridiagonal solve in the x-local layout)
    int Nxl, Nxe, Nxh, Nxg, Ny, Nyh, Nyc, Nyp, Nz;
    size_t nz_c;                // complex elements of the local paired array  Nxh*Ny*Nz
    size_t nbuf;                // complex elements of xfield / send / recv    Nxl*Nyp*Nz == Nxg*Nyc*Nz
    double2 *zfield = nullptr;  // (Nxh, Nz, Ny) complex == dense real rhs (Nxe, Nz, Ny)
    double2 *xfield = nullptr, *xsol = nullptr;   // (Nxg, Nyc, Nz)
    double2 *send = nullptr, *recv = nullptr;     // borrowed (host layer owns them: torch tensors)
    double *lam[3] = {nullptr, nullptr, nullptr};
    double *D = nullptr, *lower = nullptr, *t = nullptr;
    hipfftHandle plan_loc = 0, plan_x = 0;
    bool has_loc = false, has_x = false;
    // zmode 0, Nxg = 2^m <= 4096: the x stage (unpack, FFT, divide, inverse FFT, pack) is one LDS pass (xline_solve_kernel, ocn_line_fft.h)
    bool xfused = false;
    int logn_x = 0, xlines = 1;
    double2 *xtw = nullptr;
    // substructured x solve (see ocn_kernels.h): modes M = Nyh*Nz, spectral slab Y (M, Nxl), Thomas factors, s = T⁻¹e₀
    bool sub = false;
    long M = 0;
    double2 *Y = nullptr, *iface = nullptr;
    double *rden = nullptr, *cpf = nullptr, *svec = nullptr;
    double2 *payload = nullptr, *gathered = nullptr;     // borrowed (host layer: torch tensors): 2M+1 and R*(2M+1) complex
    // z-fastest variant of the substructured solve (option dist_zfirst): source term written z-fastest, unit-stride R2C along z, strided
    // y transform whose output is already in the order the Thomas sweeps want -- no Hermitian separation / re-pairing passes
    bool zfirst = false;
    int Nzh = 0, Nzp = 0;       // modes along z (Nz/2 + 1) and the row pitch they are stored with (multiple of 8: whole 128-B lines)
    double *rreal = nullptr;    // (Nz, Nxl, Ny) real
    double2 *spec = nullptr;    // (Nzp, Nxl, Ny) complex, modes m = kz + Nzh*ky at [kz + Nzp*(i + Nxl*ky)]
    hipfftHandle plan_zr2c = 0, plan_zc2r = 0;       // 2-D (y, z) D2Z / Z2D, batched over the local x index (zf_2d) ...
    hipfftHandle plan_y = 0;                         // ... or 1-D along z plus this strided 1-D y transform
    // z Bounded, Ny = 2^m <= 1024: the local y transform by strided_line_fft_kernel (ocn_line_fft.h) instead of rocFFT's 1-D strided plan
    bool yline = false;
    int logn_y = 0;
    double2 *ytw = nullptr;
    bool zf_2d = false;
    bool has_zf = false;
    // x-fastest variant of the substructured solve (ocn_kernels.h, "xfast"): dense real array rx (Nx, Ny, Nz), spectrum xs (Nx, Ny, Nz/2 + 1),
    // Thomas factors rden_x in the spectrum's layout, first / last entry of s = T⁻¹e₀ per mode
    bool xfast = false;
    bool src_in_spectrum = false;   // the fused source-term + z transform already filled xs: forward_local skips its z transform
    int xE = 0, logn_z = 0;
    double *rx = nullptr, *rden_x = nullptr, *s_first = nullptr, *s_last = nullptr;
    double2 *xs = nullptr, *ztw = nullptr;
};

extern "C" int ocn_dist_poisson_destroy(ocn_dist_poisson_t s) {
    if (!s) return OCN_OK;
    if (s->has_loc) hipfftDestroy(s->plan_loc);
    if (s->has_x) hipfftDestroy(s->plan_x);
    hipFree(s->zfield); hipFree(s->xfield); hipFree(s->xsol); hipFree(s->xtw);
    hipFree(s->Y); hipFree(s->iface); hipFree(s->rden); hipFree(s->cpf); hipFree(s->svec);
    hipFree(s->D); hipFree(s->lower); hipFree(s->t);
    for (int d = 0; d < 3; ++d) hipFree(s->lam[d]);
    if (s->has_zf) { hipfftDestroy(s->plan_zr2c); hipfftDestroy(s->plan_zc2r); if (!s->zf_2d) hipfftDestroy(s->plan_y); }
    hipFree(s->rreal); hipFree(s->spec); hipFree(s->ytw);
    hipFree(s->rx); hipFree(s->rden_x); hipFree(s->s_first); hipFree(s->s_last); hipFree(s->xs); hipFree(s->ztw);
    delete s;
    return OCN_OK;
}

// what every layout shares: the paired-column and x-local buffers, the eigenvalues, the tridiagonal data of a Bounded z (on this rank's
// modes) and the local (y, z) | y plan -- verified by dist_verify_local_plan once the layout has set itself up, as the order has always been
static int dist_setup_common(ocn_dist_poisson_s *s, double Lx_global) {
    const DGrid &g = s->grid->d;
    HIP_TRY(dev_alloc((void **)&s->zfield, s->nz_c * sizeof(double2)));
    HIP_TRY(dev_alloc((void **)&s->xfield, s->nbuf * sizeof(double2)));
    HIP_TRY(hipMemset(s->zfield, 0, s->nz_c * sizeof(double2)));
    HIP_TRY(hipMemset(s->xfield, 0, s->nbuf * sizeof(double2)));
    const int N[3] = {s->Nxg, s->Ny, s->Nz};
    const double L[3] = {Lx_global, s->grid->L[1], s->grid->L[2]};
    std::vector<double> lam[3];
    for (int d = 0; d < 3; ++d) {
        poisson_eigenvalues(N[d], L[d], d == 2 ? g.tz : OCN_PERIODIC, lam[d]);
        HIP_TRY(dev_alloc((void **)&s->lam[d], N[d] * sizeof(double)));
        HIP_TRY(hipMemcpy(s->lam[d], lam[d].data(), N[d] * sizeof(double), hipMemcpyHostToDevice));
    }
    if (s->zmode == 1) {
        HIP_TRY(dev_alloc((void **)&s->xsol, s->nbuf * sizeof(double2)));
        HIP_TRY(hipMemset(s->xsol, 0, s->nbuf * sizeof(double2)));
        HIP_TRY(dev_alloc((void **)&s->D, s->nbuf * sizeof(double)));
        HIP_TRY(dev_alloc((void **)&s->t, s->nbuf * sizeof(double)));
        HIP_TRY(hipMemset(s->t, 0, s->nbuf * sizeof(double)));
        { int rc_ = upload_tridiagonal_lower(s->grid, &s->lower); if (rc_) return rc_; }
        std::vector<double> D(s->nbuf);
        for (int jl = 0; jl < s->Nyc; ++jl) {
            const int jg = std::min(s->rank * s->Nyc + jl, s->Ny - 1);
            for (int i = 0; i < s->Nxg; ++i) {
                const double lxy = lam[0][i] + lam[1][jg];
                double *col = &D[(size_t)i + (size_t)s->Nxg * jl];
                if (s->Nz == 1) col[0] = -s->grid->h_dzc[g.Hz] * lxy;      // see tridiagonal_column
                else            tridiagonal_column(s->grid, lxy, col, (size_t)s->Nxg * s->Nyc);
            }
        }
        HIP_TRY(hipMemcpy(s->D, D.data(), s->nbuf * sizeof(double), hipMemcpyHostToDevice));
    }
    hipfftResult r;
    if (s->zmode == 0) {
        // (y, z) transform of (Nxh, Nz, Ny): z stride Nxh, y stride Nxh*Nz, one batch entry per column pair
        int nyz[2] = {s->Ny, s->Nz};
        r = hipfftPlanMany(&s->plan_loc, 2, nyz, nyz, s->Nxh, 1, nyz, s->Nxh, 1, HIPFFT_Z2Z, s->Nxh);
    } else {
        int ny[1] = {s->Ny};
        r = hipfftPlanMany(&s->plan_loc, 1, ny, ny, s->Nxh * s->Nz, 1, ny, s->Nxh * s->Nz, 1, HIPFFT_Z2Z, s->Nxh * s->Nz);
    }
    if (r != HIPFFT_SUCCESS) return fail(1000 + (int)r, "hipfftPlanMany(local y/z) failed (%d)", (int)r);
    s->has_loc = true;
    return OCN_OK;
}

// the round-trip check of the local plan; z Bounded, Ny = 2^m <= 1024: the LDS y-line kernel takes the plan's place at step time if it
// reproduces it
static int dist_verify_local_plan(ocn_dist_poisson_s *s) {
    int rc;
    if ((rc = plan_set_stream(s->plan_loc))) return rc;
    const double sc = s->zmode == 0 ? 1.0 / ((double)s->Ny * s->Nz) : 1.0 / (double)s->Ny;
    if ((rc = verify_complex_plan(s->plan_loc, s->zfield, (long)s->nz_c, sc, "distributed local (y, z)"))) return rc;
    if (s->zmode == 1 && s->opt->dist_yline && line_length_ok(s->Ny)) {
        s->logn_y = ilog2(s->Ny);
        if ((rc = upload_twiddles(s->Ny, &s->ytw))) return rc;
        return line_fft_matches_plan(*s->opt, s->plan_loc, s->zfield, s->nz_c, s->ytw, (long)s->Nxh * s->Nz, s->Ny, s->logn_y, &s->yline);
    }
    return OCN_OK;
}

// ---- x-fastest layout (ocn_kernels.h "xfast"; its paired z transforms: ocn_line_fft.h) ----
static int setup_xfast(ocn_dist_poisson_s *s) {
    const DGrid &g = s->grid->d;
    s->sub = true; s->xfast = true;
    s->Nzh = s->Nz / 2 + 1;
    s->M = (long)s->Ny * s->Nzh;                                     // mode m = ky + Ny kz
    s->logn_y = ilog2(s->Ny);
    s->logn_z = ilog2(s->Nz);
    s->xE = 1;
    while (s->xE * 64 < s->Nxl) s->xE *= 2;
    const size_t nreal = (size_t)s->Nxl * s->Ny * s->Nz, nspec = (size_t)s->Nxl * s->M;
    HIP_TRY(dev_alloc((void **)&s->rx, nreal * sizeof(double)));
    HIP_TRY(dev_alloc((void **)&s->xs, nspec * sizeof(double2)));
    HIP_TRY(dev_alloc((void **)&s->rden_x, nspec * sizeof(double)));
    HIP_TRY(dev_alloc((void **)&s->s_first, (size_t)s->M * sizeof(double)));
    HIP_TRY(dev_alloc((void **)&s->s_last, (size_t)s->M * sizeof(double)));
    HIP_TRY(dev_alloc((void **)&s->iface, (2 * (size_t)s->M + 2) * sizeof(double2)));
    int rc;
    if ((rc = upload_twiddles(s->Ny, &s->ytw)) || (rc = upload_twiddles(s->Nz, &s->ztw))) return rc;
    const double a = 1.0 / (g.dx * g.dx);
    // mode m = ky + Ny kz: first eigenvalue array indexed with m % Ny, second with m / Ny; the spectrum buffer is the scratch of s
    hipLaunchKernelGGL(sub_setup_xfast_kernel, dim3((unsigned)((s->M + 255) / 256)), dim3(256), 0, g_stream, s->M, s->Ny, s->Nxl, a, s->lam[1],
                       s->lam[2], s->rden_x, s->s_first, s->s_last, (double *)(s->iface + 2 * s->M + 1), (double *)s->xs);
    HIP_TRY(hipGetLastError());
    // known-answer check of the paired z transform (a round trip cannot tell a mis-read layout from the right one): column 2c
    // carries cos(2 pi k / N), column 2c + 1 carries sin(2 pi 3 k / N): X_even[1] = N/2, X_odd[3] = -i N/2, everything else 0;
    // then the way back reproduces the input
    const long C = (long)s->Nxl * s->Ny / 2;
    DevTmp<double> bm;
    HIP_TRY(bm.alloc(2));
    hipLaunchKernelGGL(xfast_kat_fill_kernel, dim3((unsigned)((nreal / 2 + 255) / 256)), dim3(256), 0, g_stream, (double2 *)s->rx, C, s->Nz);
    launch_paired_zline(*s->opt, true, (const double2 *)s->rx, s->xs, s->ztw, C, s->Nz, s->logn_z, 1.0);
    hipLaunchKernelGGL(xfast_kat_check_kernel, dim3(1), dim3(256), 0, g_stream, (const double2 *)s->xs, C, s->Nz, bm.p);
    launch_paired_zline(*s->opt, false, s->xs, (double2 *)s->rx, s->ztw, C, s->Nz, s->logn_z, 1.0 / (double)s->Nz);
    hipLaunchKernelGGL(xfast_kat_check_real_kernel, dim3(1), dim3(256), 0, g_stream, (const double2 *)s->rx, C, s->Nz, bm.p + 1);
    double err[2] = {1.0, 1.0};
    hipError_t e_ = hipMemcpyAsync(err, bm.p, sizeof(err), hipMemcpyDeviceToHost, g_stream);
    if (e_ == hipSuccess) e_ = hipStreamSynchronize(g_stream);
    if (e_ != hipSuccess) return fail((int)e_, "x-fastest solver self-check: %s", hipGetErrorString(e_));
    if (!(err[0] < 1e-10 * s->Nz) || !(err[1] < 1e-12 * s->Nz))
        return fail(OCN_EFFT, "the paired z line transform failed its known-answer check (spectrum %.3g, round trip %.3g)", err[0], err[1]);
    return OCN_OK;
}

// ---- z-fastest layout ----
// a round trip cannot tell a transform of a mis-read layout from the right one: the 2-D plan's spectrum against plain 1-D plans, once
// (pseudo-random data); the 1-D plans are dropped afterwards
static int zfirst_check_2d_plan(ocn_dist_poisson_s *s, size_t pslab) {
    hipfftHandle pz = 0, py = 0;
    int nz1[1] = {s->Nz}, ny1[1] = {s->Ny}, rez2[1] = {s->Nz}, cez2[1] = {s->Nzp};
    DevTmp<double2> ref;
    DevTmp<double> bm;
    const long nreal = (long)s->Nz * s->Nxl * s->Ny;
    hipfftResult r1 = hipfftPlanMany(&pz, 1, nz1, rez2, 1, s->Nz, cez2, 1, s->Nzp, HIPFFT_D2Z, s->Nxl * s->Ny);
    hipfftResult r2 = r1 == HIPFFT_SUCCESS ? hipfftPlanMany(&py, 1, ny1, ny1, s->Nzp * s->Nxl, 1, ny1, s->Nzp * s->Nxl, 1, HIPFFT_Z2Z, s->Nzp * s->Nxl) : r1;
    bool ok = r1 == HIPFFT_SUCCESS && r2 == HIPFFT_SUCCESS && ref.alloc(pslab) == hipSuccess && bm.alloc(256) == hipSuccess;
    double err = -1.0;
    if (ok) {
        hipfftSetStream(pz, g_stream); hipfftSetStream(py, g_stream);
        hipLaunchKernelGGL(selfcheck_fill_real, dim3((unsigned)((nreal + 255) / 256)), dim3(256), 0, g_stream, s->rreal, nreal);
        ok = hipMemsetAsync(ref.p, 0, pslab * sizeof(double2), g_stream) == hipSuccess && hipfftExecD2Z(pz, s->rreal, (hipfftDoubleComplex *)ref.p) == HIPFFT_SUCCESS &&
             hipfftExecZ2Z(py, (hipfftDoubleComplex *)ref.p, (hipfftDoubleComplex *)ref.p, HIPFFT_FORWARD) == HIPFFT_SUCCESS &&
             hipfftExecD2Z(s->plan_zr2c, s->rreal, (hipfftDoubleComplex *)s->spec) == HIPFFT_SUCCESS;
        if (ok) {
            hipLaunchKernelGGL(max_abs_diff_kernel, dim3(256), dim3(256), 0, g_stream, (const double *)ref.p, (const double *)s->spec, 2 * (long)pslab, bm.p);
            ok = reduce_blockmax(bm.p, 256, &err) == OCN_OK;
        }
    }
    if (pz) hipfftDestroy(pz);
    if (py) hipfftDestroy(py);
    if (!ok || !(err >= 0.0 && err < 1e-9 * (double)s->Ny * (double)s->Nz))
        return fail(OCN_EFFT, "the 2-D (y, z) real plan disagrees with 1-D plans (max difference %.3g): refusing it", err);
    return OCN_OK;
}

// real pair: fill, R2C, C2R, compare
static int zfirst_verify_real_pair(ocn_dist_poisson_s *s) {
    const long n = (long)s->Nz * s->Nxl * s->Ny;
    const int nb = 256;
    DevTmp<double> bm;
    HIP_TRY(bm.alloc(nb));
    hipLaunchKernelGGL(selfcheck_fill_real, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, g_stream, s->rreal, n);
    hipfftResult r1 = hipfftExecD2Z(s->plan_zr2c, s->rreal, (hipfftDoubleComplex *)s->spec);
    if (r1 == HIPFFT_SUCCESS) r1 = hipfftExecZ2D(s->plan_zc2r, (hipfftDoubleComplex *)s->spec, s->rreal);
    hipLaunchKernelGGL(selfcheck_compare_real, dim3(nb), dim3(256), 0, g_stream, s->rreal, s->Nz, s->Nxl, s->Ny, s->Nz, s->Nxl, 0, 0, 0,
                       s->zf_2d ? 1.0 / ((double)s->Nz * (double)s->Ny) : 1.0 / (double)s->Nz, bm.p);
    double err = 0;
    const int rc = r1 == HIPFFT_SUCCESS ? reduce_blockmax(bm.p, nb, &err) : fail(1000 + (int)r1, "hipFFT exec failed in the plan self-check (%d)", (int)r1);
    if (rc) return rc;
    if (!(err < 1e-10)) return fail(OCN_EFFT, "rocFFT self-check failed for the (y, z) real transform pair (round-trip error %.3g)", err);
    return OCN_OK;
}

static int setup_zfirst(ocn_dist_poisson_s *s) {
    const DGrid &g = s->grid->d;
    s->sub = true; s->zfirst = true;
    s->Nzh = s->Nz / 2 + 1;
    s->Nzp = (s->Nzh + 7) & ~7;
    s->M = (long)s->Nzh * s->Ny;
    const size_t slab = (size_t)s->M * s->Nxl;                       // factor arrays: mode-fastest, unpadded
    const size_t pslab = (size_t)s->Nzp * s->Nxl * s->Ny;            // the spectrum itself: padded rows
    HIP_TRY(dev_alloc((void **)&s->rreal, (size_t)s->Nz * s->Nxl * s->Ny * sizeof(double)));
    HIP_TRY(dev_alloc((void **)&s->spec, pslab * sizeof(double2)));
    HIP_TRY(hipMemset(s->spec, 0, pslab * sizeof(double2)));
    HIP_TRY(dev_alloc((void **)&s->rden, slab * sizeof(double)));
    HIP_TRY(dev_alloc((void **)&s->cpf, slab * sizeof(double)));
    HIP_TRY(dev_alloc((void **)&s->svec, slab * sizeof(double)));
    HIP_TRY(dev_alloc((void **)&s->iface, (2 * (size_t)s->M + 2) * sizeof(double2)));
    const double a = 1.0 / (g.dx * g.dx);
    // mode m = kz + Nzh*ky: the setup kernel indexes its first eigenvalue array with m % n and the second with m / n
    hipLaunchKernelGGL(sub_setup_kernel, dim3((unsigned)((s->M + 255) / 256)), dim3(256), 0, g_stream, (int)s->M, s->Nzh, s->Nxl, a,
                       s->lam[2], s->lam[1], s->rden, s->cpf, s->svec, (double *)(s->iface + 2 * s->M + 1));
    HIP_TRY(hipGetLastError());
    // ONE 2-D real plan over (y, z) per direction, the local x index as the batch in the middle of the layout: row pitch
    // Nz*Nxl (Nzh*Nxl on the complex side), batch distance Nz (Nzh). As a 2-D plan rocFFT runs the strided y pass with its
    // column kernel; the same pass as a 1-D strided plan gets the 3x slower row kernel (measured: 280 vs 90 us).
    int nyz[2] = {s->Ny, s->Nz};
    int remb[2] = {s->Ny, s->Nz * s->Nxl}, cemb[2] = {s->Ny, s->Nzp * s->Nxl};
    // ... unless Ny = 2^m <= 1024: then the y pass is strided_line_fft_kernel (3x faster again than the column kernel of the 2-D
    // plan) next to plain 1-D plans along z
    const bool want_yline = s->opt->dist_yline && line_length_ok(s->Ny);
    hipfftResult rz = want_yline ? HIPFFT_NOT_SUPPORTED
                                 : hipfftPlanMany(&s->plan_zr2c, 2, nyz, remb, 1, s->Nz, cemb, 1, s->Nzp, HIPFFT_D2Z, s->Nxl);
    if (rz == HIPFFT_SUCCESS) {
        rz = hipfftPlanMany(&s->plan_zc2r, 2, nyz, cemb, 1, s->Nzp, remb, 1, s->Nz, HIPFFT_Z2D, s->Nxl);
        if (rz != HIPFFT_SUCCESS) { hipfftDestroy(s->plan_zr2c); s->plan_zr2c = 0; }
    }
    s->zf_2d = rz == HIPFFT_SUCCESS;
    int rc;
    if (!s->zf_2d) {
        // rocFFT refuses the interleaved-batch 2-D layout for some (small) sizes: 1-D R2C along z + 1-D strided y transform
        (void)hipGetLastError();
        int nz1[1] = {s->Nz}, ny1[1] = {s->Ny}, rez[1] = {s->Nz}, cez[1] = {s->Nzp};
        rz = hipfftPlanMany(&s->plan_zr2c, 1, nz1, rez, 1, s->Nz, cez, 1, s->Nzp, HIPFFT_D2Z, s->Nxl * s->Ny);
        if (rz == HIPFFT_SUCCESS) rz = hipfftPlanMany(&s->plan_zc2r, 1, nz1, cez, 1, s->Nzp, rez, 1, s->Nz, HIPFFT_Z2D, s->Nxl * s->Ny);
        if (rz == HIPFFT_SUCCESS)
            rz = hipfftPlanMany(&s->plan_y, 1, ny1, ny1, s->Nzp * s->Nxl, 1, ny1, s->Nzp * s->Nxl, 1, HIPFFT_Z2Z, s->Nzp * s->Nxl);
        if (rz != HIPFFT_SUCCESS) return fail(1000 + (int)rz, "hipfftPlanMany(z-fastest local transforms) failed (%d)", (int)rz);
        if ((rc = plan_set_stream(s->plan_y))) return rc;
        if ((rc = verify_complex_plan(s->plan_y, s->spec, (long)pslab, 1.0 / (double)s->Ny, "distributed y (z-fastest layout)"))) return rc;
        if (want_yline) {
            s->logn_y = ilog2(s->Ny);
            if ((rc = upload_twiddles(s->Ny, &s->ytw))) return rc;
            if ((rc = line_fft_matches_plan(*s->opt, s->plan_y, s->spec, pslab, s->ytw, (long)s->Nzp * s->Nxl, s->Ny, s->logn_y, &s->yline))) return rc;
        }
    }
    HIP_TRY(hipMemsetAsync(s->spec, 0, pslab * sizeof(double2), g_stream));     // the self-checks wrote into the padding
    s->has_zf = true;
    if ((rc = plan_set_stream(s->plan_zr2c)) || (rc = plan_set_stream(s->plan_zc2r))) return rc;
    if (s->zf_2d && (rc = zfirst_check_2d_plan(s, pslab))) return rc;
    return zfirst_verify_real_pair(s);
}

// ---- paired-column layout ----
static int setup_paired(ocn_dist_poisson_s *s) {
    const DGrid &g = s->grid->d;
    s->sub = true;
    s->M = (long)s->Nyh * s->Nz;
    const size_t slab = (size_t)s->M * s->Nxl;
    HIP_TRY(dev_alloc((void **)&s->Y, slab * sizeof(double2)));
    HIP_TRY(dev_alloc((void **)&s->rden, slab * sizeof(double)));
    HIP_TRY(dev_alloc((void **)&s->cpf, slab * sizeof(double)));
    HIP_TRY(dev_alloc((void **)&s->svec, slab * sizeof(double)));
    HIP_TRY(dev_alloc((void **)&s->iface, (2 * (size_t)s->M + 2) * sizeof(double2)));      // + one slot: Σ s of the null mode
    const double a = 1.0 / (g.dx * g.dx);
    hipLaunchKernelGGL(sub_setup_kernel, dim3((unsigned)((s->M + 255) / 256)), dim3(256), 0, g_stream, (int)s->M, s->Nyh, s->Nxl, a,
                       s->lam[1], s->lam[2], s->rden, s->cpf, s->svec, (double *)(s->iface + 2 * s->M + 1));
    HIP_TRY(hipGetLastError());
    return OCN_OK;
}

// ---- transposing solver: the x stage as one LDS pass (zmode 0, Nxg = 2^m <= 4096) or on a rocFFT plan ----
static int setup_fused_xline(ocn_dist_poisson_s *s) {
    s->xfused = true;
    s->logn_x = ilog2(s->Nxg);
    s->xlines = std::max(1, 4096 / s->Nxg);           // 64 KB of LDS per workgroup
    return upload_twiddles(s->Nxg, &s->xtw);
}
static int setup_x_plan(ocn_dist_poisson_s *s) {
    int nx[1] = {s->Nxg};
    hipfftResult r = hipfftPlanMany(&s->plan_x, 1, nx, nullptr, 1, s->Nxg, nullptr, 1, s->Nxg, HIPFFT_Z2Z, s->Nyc * s->Nz);
    if (r != HIPFFT_SUCCESS) return fail(1000 + (int)r, "hipfftPlanMany(x) failed (%d)", (int)r);
    s->has_x = true;
    int rc;
    if ((rc = plan_set_stream(s->plan_x))) return rc;
    return verify_complex_plan(s->plan_x, s->xfield, (long)s->nbuf, 1.0 / (double)s->Nxg, "distributed x");
}

// everything a fresh solver owns: the common part, then what the chosen layout owns; on an error the caller destroys the half-built solver
static int dist_poisson_setup(ocn_dist_poisson_s *s, double Lx_global) {
    const OcnOptions *opt = s->opt;
    const int zmode = s->zmode;
    int rc;
    if ((rc = dist_setup_common(s, Lx_global))) return rc;
    if (zmode == 0 && opt->dist_substructured && opt->dist_xfast && (s->Nxl % 2) == 0 && s->Nxl <= 1024 && line_length_ok(s->Ny) && line_length_ok(s->Nz))
        rc = setup_xfast(s);
    else if (zmode == 0 && opt->dist_substructured && opt->dist_zfirst)
        rc = setup_zfirst(s);
    else if (zmode == 0 && opt->dist_substructured)
        rc = setup_paired(s);
    if (rc) return rc;
    if (!s->sub && zmode == 0 && opt->fused_zfft && line_length_ok(s->Nxg, 4096) && (rc = setup_fused_xline(s))) return rc;
    if ((rc = dist_verify_local_plan(s))) return rc;
    if (!s->xfused && !s->sub) return setup_x_plan(s);
    return OCN_OK;
}

static int dist_poisson_create(ocn_dist_poisson_t *solver, ocn_grid_t local_grid, int R, int rank, double Lx_global, const OcnOptions *opt) {
    NEED_INIT();
    if (!solver || !local_grid) return fail(OCN_EINVAL, "NULL argument");
    const DGrid &g = local_grid->d;
    if (R < 1 || rank < 0 || rank >= R) return fail(OCN_EINVAL, "invalid rank %d of %d", rank, R);
    // (one rank with a FullyConnected x is its own neighbour on both sides: the N > 1 code path measured on one GPU)
    if (g.ty != OCN_PERIODIC || (R > 1 && g.tx != OCN_CONNECTED) || (R == 1 && g.tx != OCN_PERIODIC && g.tx != OCN_CONNECTED))
        return fail(OCN_ENOTSUP, "the distributed Poisson solvers are accelerated for (Periodic, Periodic, Periodic | Bounded) x-slab partitions");
    // validate_poisson_solver_distributed_grid (:194-229): Ny must be divisible by Rx
    if (g.Ny % R != 0) return fail(OCN_EINVAL, "Ny = %d must be divisible by the number of ranks %d (transpose y -> x)", g.Ny, R);
    const int zmode = g.tz == OCN_BOUNDED ? 1 : 0;
    if (zmode == 0 && !local_grid->z_regular) return fail(OCN_EINVAL, "DistributedFFTBasedPoissonSolver requires a regular grid");
    ocn_dist_poisson_s *s = new ocn_dist_poisson_s();
    s->grid = local_grid; s->opt = opt; s->R = R; s->rank = rank; s->zmode = zmode;
    s->Nxl = g.Nx; s->Nxe = g.Nx + (g.Nx & 1); s->Nxh = s->Nxe / 2; s->Nxg = g.Nx * R;
    s->Ny = g.Ny; s->Nyh = g.Ny / 2 + 1; s->Nyc = (s->Nyh + R - 1) / R; s->Nyp = s->Nyc * R; s->Nz = g.Nz;
    s->nz_c = (size_t)s->Nxh * s->Ny * s->Nz;
    s->nbuf = (size_t)s->Nxg * s->Nyc * s->Nz;
    const int rc = dist_poisson_setup(s, Lx_global);
    if (rc) { ocn_dist_poisson_destroy(s); return rc; }
    *solver = s;
    return OCN_OK;
}
extern "C" int ocn_dist_poisson_create(ocn_dist_poisson_t *solver, ocn_grid_t local_grid, int R, int rank, double Lx_global) {
    return dist_poisson_create(solver, local_grid, R, rank, Lx_global, &g_defaults);
}

extern "C" int ocn_dist_poisson_buffer_size(ocn_dist_poisson_t s, size_t *complex_elements) {
    if (!s || !complex_elements) return fail(OCN_EINVAL, "NULL argument");
    *complex_elements = s->nbuf;
    return OCN_OK;
}

// 0: paired-column layout; 1: z-fastest layout with 1-D plans; 2: z-fastest layout with the 2-D (y, z) real plans; 3: z-fastest with the LDS
// y-line kernel; 4: x-fastest layout (paired z transform in LDS, Thomas scans); -1 transposing solver
extern "C" int ocn_dist_poisson_layout(ocn_dist_poisson_t s, int *layout) {
    if (!s || !layout) return fail(OCN_EINVAL, "NULL argument");
    *layout = !s->sub ? -1 : (s->xfast ? 4 : (!s->zfirst ? 0 : (s->yline ? 3 : (s->zf_2d ? 2 : 1))));
    return OCN_OK;
}

// substructured mode: complex elements of the per-rank payload (first / last value per mode + the null mode's sum); 0 otherwise
extern "C" int ocn_dist_poisson_payload_size(ocn_dist_poisson_t s, size_t *complex_elements) {
    if (!s || !complex_elements) return fail(OCN_EINVAL, "NULL argument");
    *complex_elements = s->sub ? 2 * (size_t)s->M + 1 : 0;
    return OCN_OK;
}

extern "C" int ocn_dist_poisson_set_gather_buffers(ocn_dist_poisson_t s, double *payload_complex, double *gathered_complex) {
    if (!s || !payload_complex || !gathered_complex) return fail(OCN_EINVAL, "NULL argument");
    if (!s->sub) return fail(OCN_ESTATE, "this solver transposes (all-to-all); it has no gather buffers");
    s->payload = (double2 *)payload_complex; s->gathered = (double2 *)gathered_complex;
    return OCN_OK;
}

// substructured mode, stage 1: local (y, z) transform, column separation, Thomas sweeps along x, payload. Afterwards the host layer
// runs all_gather(gathered, payload).
extern "C" int ocn_dist_poisson_forward_local(ocn_dist_poisson_t s) {
    NEED_INIT();
    if (!s || !s->sub || !s->payload) return fail(OCN_EINVAL, "substructured solver / gather buffers not set");
    int rc;
    const double a = 1.0 / (s->grid->d.dx * s->grid->d.dx);
    if (s->xfast) {
        const long C = (long)s->Nxl * s->Ny / 2, P = (long)s->Nxl * s->Ny;
        if (!s->src_in_spectrum) launch_paired_zline(*s->opt, true, (const double2 *)s->rx, s->xs, s->ztw, C, s->Nz, s->logn_z, 1.0);
        s->src_in_spectrum = false;
        launch_strided_line_fft(*s->opt, s->xs, s->ytw, (long)s->Nxl, (long)s->Nxl, (unsigned)s->Nzh, s->Ny, s->logn_y, 0, 1.0, P);
        launch_xline_thomas<false>(*s->opt, s->xE, s->xs, s->rden_x, s->M, s->Nxl, a, s->payload, nullptr, 1.0);      // reads only: the payload
        KERNEL_CHECK();
        return OCN_OK;
    }
    if (s->zfirst) {
        if ((rc = plan_set_stream(s->plan_zr2c))) return rc;
        FFT_TRY(hipfftExecD2Z(s->plan_zr2c, s->rreal, (hipfftDoubleComplex *)s->spec));
        if (s->yline) {
            const long C = (long)s->Nzp * s->Nxl;
            launch_strided_line_fft(*s->opt, s->spec, s->ytw, C, C, 1, s->Ny, s->logn_y, 0, 1.0);
        } else if (!s->zf_2d) {
            if ((rc = plan_set_stream(s->plan_y))) return rc;
            FFT_TRY(hipfftExecZ2Z(s->plan_y, (hipfftDoubleComplex *)s->spec, (hipfftDoubleComplex *)s->spec, HIPFFT_FORWARD));
        }
        hipLaunchKernelGGL(sub_thomas_kernel<true>, dim3((unsigned)((s->M + 63) / 64)), dim3(64), 0, g_stream, s->M, s->Nxl, a, s->rden, s->cpf,
                           s->spec, s->payload, s->Nzh, s->Nzp);
        KERNEL_CHECK();
        return OCN_OK;
    }
    if ((rc = plan_set_stream(s->plan_loc))) return rc;
    FFT_TRY(hipfftExecZ2Z(s->plan_loc, (hipfftDoubleComplex *)s->zfield, (hipfftDoubleComplex *)s->zfield, HIPFFT_FORWARD));
    const dim3 blk(16, 16), grd((s->Nxh + 15) / 16, (s->Nyh + 15) / 16, s->Nz);
    hipLaunchKernelGGL(sub_separate_kernel, grd, blk, 0, g_stream, s->zfield, s->Y, s->Nxl, s->Nxh, s->Ny, s->Nyh, s->Nz);
    hipLaunchKernelGGL(sub_thomas_kernel<false>, dim3((unsigned)((s->M + 63) / 64)), dim3(64), 0, g_stream, s->M, s->Nxl, a, s->rden, s->cpf, s->Y,
                       s->payload, 1, 1);
    KERNEL_CHECK();
    return OCN_OK;
}

// the paired-column real array of the transposing solvers and of the substructured solver's layout 0: (x, z, y), rows of Nxe
static DenseLayout dist_paired_columns(const ocn_dist_poisson_s *s) { return {(long)s->Nxe * s->Nz, (long)s->Nxe}; }
// where the solver leaves its dense x-fastest solution (not the z-fastest layouts: s->rreal, read by their own kernels)
static DenseSolution dist_dense_solution(const ocn_dist_poisson_s *s) {
    if (s->xfast) return {(const double *)s->rx, DenseLayout{}.on(s->grid->d)};
    return {(const double *)s->zfield, dist_paired_columns(s)};
}

// substructured mode, stage 2: interface unknowns from the gathered payloads, slab correction, rebuild the paired spectrum,
// inverse local transform, copy into the haloed pressure
// keep_zfast (z-fastest layout only): leave the solution in the solver's dense z-fastest real array (s->rreal) instead of copying it
// into a haloed field -- the partitioned model's pressure correction reads it there (pressure_correction_zfast_kernel)
static int dist_poisson_backward_local(ocn_dist_poisson_t s, double *phi, bool keep_zfast) {
    const DGrid &g = s->grid->d;
    const double a = 1.0 / (g.dx * g.dx);
    const double scale = 1.0 / ((double)s->Ny * (double)s->Nz);
    if (s->xfast) {
        // interface unknowns, then the SAME line solve on the right-hand side that carries them in its two end entries: the final solution
        hipLaunchKernelGGL(sub_interface_kernel, dim3((unsigned)((s->M + 255) / 256)), dim3(256), 0, g_stream, s->M, s->Ny, s->Nxl, s->R, s->rank,
                           a, s->lam[1], s->lam[2], s->s_first, s->s_last, (const double *)(s->iface + 2 * s->M + 1), s->gathered, s->iface);
        launch_xline_thomas<true>(*s->opt, s->xE, s->xs, s->rden_x, s->M, s->Nxl, a, nullptr, s->iface, scale);
        const long C = (long)s->Nxl * s->Ny / 2, P = (long)s->Nxl * s->Ny;
        launch_strided_line_fft(*s->opt, s->xs, s->ytw, (long)s->Nxl, (long)s->Nxl, (unsigned)s->Nzh, s->Ny, s->logn_y, 1, 1.0, P);
        launch_paired_zline(*s->opt, false, s->xs, (double2 *)s->rx, s->ztw, C, s->Nz, s->logn_z, 1.0);
        if (!keep_zfast && !phi) return fail(OCN_EINVAL, "NULL pressure field");
        if (!keep_zfast)           // (here: keep the dense x-fastest solution in s->rx)
            launch_copy_dense_to_field(g, phi, dist_dense_solution(s));
        KERNEL_CHECK();
        return OCN_OK;
    }
    hipLaunchKernelGGL(sub_interface_kernel, dim3((unsigned)((s->M + 255) / 256)), dim3(256), 0, g_stream, s->M, s->Nyh, s->Nxl, s->R, s->rank,
                       a, s->lam[1], s->lam[2], s->svec, s->svec + s->M * (long)(s->Nxl - 1), (const double *)(s->iface + 2 * s->M + 1), s->gathered, s->iface);
    if (s->zfirst) {
        const long total = (long)s->Nzp * s->Nxl * s->Ny;
        hipLaunchKernelGGL(sub_correct_zfast_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, g_stream, s->spec, s->svec, s->iface,
                           s->M, s->Nxl, s->Nzh, s->Ny, a, scale, s->Nzp);
        int rcz;
        if (s->yline) {
            const long C = (long)s->Nzp * s->Nxl;
            launch_strided_line_fft(*s->opt, s->spec, s->ytw, C, C, 1, s->Ny, s->logn_y, 1, 1.0);
        } else if (!s->zf_2d) {
            if ((rcz = plan_set_stream(s->plan_y))) return rcz;
            FFT_TRY(hipfftExecZ2Z(s->plan_y, (hipfftDoubleComplex *)s->spec, (hipfftDoubleComplex *)s->spec, HIPFFT_BACKWARD));
        }
        if ((rcz = plan_set_stream(s->plan_zc2r))) return rcz;
        FFT_TRY(hipfftExecZ2D(s->plan_zc2r, (hipfftDoubleComplex *)s->spec, s->rreal));
        if (!keep_zfast && !phi) return fail(OCN_EINVAL, "NULL pressure field");
        if (!keep_zfast)
            hipLaunchKernelGGL(copy_real_zfast_kernel, dim3((g.Nx + 31) / 32, (g.Nz + 31) / 32, g.Ny), dim3(32, 8), 0, g_stream, g,
                               make_view(g, phi, LOC_C), s->rreal);
        KERNEL_CHECK();
        return OCN_OK;
    }
    const dim3 blk(16, 16), grd((s->Nxh + 15) / 16, (s->Nyh + 15) / 16, s->Nz);
    hipLaunchKernelGGL(sub_correct_combine_kernel, grd, blk, 0, g_stream, s->Y, s->svec, s->iface, s->zfield, s->Nxl, s->Nxh, s->Ny, s->Nyh,
                       s->Nz, a, scale);
    int rc;
    if ((rc = plan_set_stream(s->plan_loc))) return rc;
    FFT_TRY(hipfftExecZ2Z(s->plan_loc, (hipfftDoubleComplex *)s->zfield, (hipfftDoubleComplex *)s->zfield, HIPFFT_BACKWARD));
    if (!phi) return fail(OCN_EINVAL, "this layout of the substructured solver writes the haloed pressure field: NULL given");
    launch_copy_dense_to_field(g, phi, dist_dense_solution(s));
    KERNEL_CHECK();
    return OCN_OK;
}
extern "C" int ocn_dist_poisson_backward_local(ocn_dist_poisson_t s, double *phi) {
    NEED_INIT();
    if (!s || !s->sub || !s->gathered || !phi) return fail(OCN_EINVAL, "substructured solver / gather buffers not set");
    return dist_poisson_backward_local(s, phi, false);
}

extern "C" int ocn_dist_poisson_set_buffers(ocn_dist_poisson_t s, double *send_complex, double *recv_complex) {
    if (!s || !send_complex || !recv_complex) return fail(OCN_EINVAL, "NULL argument");
    s->send = (double2 *)send_complex; s->recv = (double2 *)recv_complex;
    return OCN_OK;
}

// compute_source_term! into the solver's paired-column real storage (solve_for_pressure.jl:12-84; weighted by Δzᶜ for the
// tridiagonal solver)
extern "C" int ocn_dist_poisson_source_term(ocn_dist_poisson_t s, const double *u, const double *v, const double *w) {
    NEED_INIT();
    if (!s || !u || !v || !w) return fail(OCN_EINVAL, "NULL argument");
    if (s->xfast) return source_term(s->grid->d, u, v, w, s->rx, false, true);
    if (s->zfirst) return source_term_zfast(s->grid->d, u, v, w, s->rreal);
    return source_term(s->grid->d, u, v, w, s->zfield, s->zmode == 1, true, SourceLayout{dist_paired_columns(s), s->Nxe != s->Nxl});
}

// the partitioned model's form (z-fastest layout): no halo is read -- y / z neighbours at wrapped interior indices, u[Nx+1] from `u_east`, the
// (Ny, Nz) column received by the one-column exchange
static int dist_poisson_source_term_wrapped(ocn_dist_poisson_t s, const double *u, const double *v, const double *w, const double *u_east) {
    const DGrid &g = s->grid->d;
    if (s->xfast && s->opt->dist_fuse_source) {
        const long C = (long)s->Nxl * s->Ny / 2;
        const int zl = line_zl(*s->opt, s->Nz);
        const dim3 grd((unsigned)((C + zl - 1) / zl));
        const size_t lds = (size_t)s->Nz * zl * sizeof(double2);
        const FView fu = make_view(g, u, LOC_U), fv = make_view(g, v, LOC_V), fw = make_view(g, w, LOC_W);
        with_line_count(zl, [&](auto ZL) {
            hipLaunchKernelGGL(source_paired_zline_r2c_kernel<decltype(ZL)::value>, grd, dim3(256), lds, g_stream, g, fu, fv, fw, u_east, s->xs, s->ztw, C, s->Nz, s->logn_z);
        });
        KERNEL_CHECK();
        s->src_in_spectrum = true;
        return OCN_OK;
    }
    if (s->xfast) return source_term(g, u, v, w, s->rx, false, true, SourceLayout{{}, false, 6, u_east});
    if (!s->zfirst)     // transposing solvers (paired-column layout): y wraps (Periodic), z wraps when Periodic; a Bounded z reads its wall faces
        return source_term(g, u, v, w, s->zfield, s->zmode == 1, true,
                           SourceLayout{dist_paired_columns(s), s->Nxe != s->Nxl, 2 | (s->zmode == 0 ? 4 : 0), u_east});
    return source_term_zfast(g, u, v, w, s->rreal, u_east);
}

static int transpose_stage(ocn_dist_poisson_s *s, int dir, const double2 *src, double2 *dst) {
    const long total = (long)s->nbuf;
    hipLaunchKernelGGL(transpose_stage_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, g_stream, dir, s->R, s->Nxl, s->Nyc,
                       s->Nz, src, dst);
    KERNEL_CHECK();
    return OCN_OK;
}

// stage 1: local forward transform (:148-151), separate the column pairs and pack for transpose_y_to_x!. Afterwards the
// host layer runs all_to_all(recv, send).
extern "C" int ocn_dist_poisson_forward_yz(ocn_dist_poisson_t s) {
    NEED_INIT();
    if (!s || !s->send) return fail(OCN_EINVAL, "solver / buffers not set");
    int rc;
    if (s->yline) {
        const long C = (long)s->Nxh * s->Nz;
        launch_strided_line_fft(*s->opt, s->zfield, s->ytw, C, C, 1, s->Ny, s->logn_y, 0, 1.0);
    } else {
        if ((rc = plan_set_stream(s->plan_loc))) return rc;
        FFT_TRY(hipfftExecZ2Z(s->plan_loc, (hipfftDoubleComplex *)s->zfield, (hipfftDoubleComplex *)s->zfield, HIPFFT_FORWARD));
    }
    hipLaunchKernelGGL(dist_pack_forward_kernel, grid3(s->Nxh, s->Nyp, s->Nz, BLK), BLK, 0, g_stream, s->zfield, s->send, s->Nxl, s->Nxh,
                       s->Ny, s->Nyh, s->Nyc, s->Nyp, s->Nz, s->zmode == 0);
    KERNEL_CHECK();
    return OCN_OK;
}

// stage 2: unpack into the x-local layout, forward FFT in x, spectral divide | tridiagonal solve, backward FFT in x
// (:152-166), pack for transpose_x_to_y!. Afterwards the host layer runs all_to_all(recv, send) again.
extern "C" int ocn_dist_poisson_solve_x(ocn_dist_poisson_t s) {
    NEED_INIT();
    if (!s || !s->send) return fail(OCN_EINVAL, "solver / buffers not set");
    int rc;
    if (s->xfused) {
        // send may alias recv (one rank): a workgroup reads all of its lines before it writes them back
        const double scale = 1.0 / ((double)s->Nxg * (double)s->Ny * (double)s->Nz);
        const long nlines = (long)s->Nyc * s->Nz;
        const unsigned nb = (unsigned)((nlines + s->xlines - 1) / s->xlines);
        hipLaunchKernelGGL(xline_solve_kernel, dim3(nb), dim3(256), (size_t)s->xlines * s->Nxg * sizeof(double2), g_stream, s->recv, s->send,
                           s->xtw, s->lam[0], s->lam[1], s->lam[2], s->R, s->Nxl, s->Nyc, s->Nz, s->logn_x, s->xlines, s->rank * s->Nyc,
                           s->Ny, scale);
        KERNEL_CHECK();
        return OCN_OK;
    }
    if ((rc = transpose_stage(s, 1, s->recv, s->xfield))) return rc;
    if ((rc = plan_set_stream(s->plan_x))) return rc;
    FFT_TRY(hipfftExecZ2Z(s->plan_x, (hipfftDoubleComplex *)s->xfield, (hipfftDoubleComplex *)s->xfield, HIPFFT_FORWARD));
    double2 *sol = s->xfield;
    if (s->zmode == 0) {
        const double scale = 1.0 / ((double)s->Nxg * (double)s->Ny * (double)s->Nz);
        hipLaunchKernelGGL(dist_spectral_divide_kernel, grid3(s->Nxg, s->Nyc, s->Nz, BLK), BLK, 0, g_stream, s->xfield, s->lam[0],
                           s->lam[1], s->lam[2], s->Nxg, s->Nyc, s->Nz, s->rank * s->Nyc, s->Ny, scale);
    } else {
        const double scale = 1.0 / ((double)s->Nxg * (double)s->Ny);
        hipLaunchKernelGGL(tridiagonal_z_kernel, dim3((s->Nxg + 63) / 64, s->Nyc), dim3(64), 0, g_stream, s->Nxg, s->Nxg, s->Nyc, s->Nz,
                           s->lower, s->D, s->lower, s->xfield, s->t, s->xsol, scale, true);
        // the serial solver subtracts the mean (fourier_tridiagonal_poisson_solver.jl:233); the reference's distributed
        // solver does not -- the difference is a constant in p, which only its gradient uses. Kept identical to the
        // single-GPU path: the (0, 0) column lives on rank 0.
        if (s->rank == 0)
            hipLaunchKernelGGL(remove_mean_mode_kernel, dim3(1), dim3(256), 0, g_stream, s->xsol, (long)s->Nxg * s->Nyc, s->Nz);
        sol = s->xsol;
    }
    FFT_TRY(hipfftExecZ2Z(s->plan_x, (hipfftDoubleComplex *)sol, (hipfftDoubleComplex *)sol, HIPFFT_BACKWARD));
    return transpose_stage(s, 2, sol, s->send);
}

// stage 3: rebuild the paired spectrum, local backward transform, copy into the haloed pressure (:167-178)
// keep_dense: leave the solution in the paired-column real array (element (i, j, k) at (i-1) + Nxe ((k-1) + Nz (j-1)) of s->zfield) for the
// partitioned model's dense pressure correction instead of copying it into a haloed field
static int dist_poisson_backward_yz(ocn_dist_poisson_t s, double *phi, bool keep_dense) {
    const DGrid &g = s->grid->d;
    int rc;
    hipLaunchKernelGGL(dist_combine_backward_kernel, grid3(s->Nxh, s->Ny, s->Nz, BLK), BLK, 0, g_stream, s->recv, s->zfield, s->Nxl, s->Nxh,
                       s->Ny, s->Nyh, s->Nyc, s->Nz, s->zmode == 0);
    if (s->yline) {
        const long C = (long)s->Nxh * s->Nz;
        launch_strided_line_fft(*s->opt, s->zfield, s->ytw, C, C, 1, s->Ny, s->logn_y, 1, 1.0);
    } else {
        if ((rc = plan_set_stream(s->plan_loc))) return rc;
        FFT_TRY(hipfftExecZ2Z(s->plan_loc, (hipfftDoubleComplex *)s->zfield, (hipfftDoubleComplex *)s->zfield, HIPFFT_BACKWARD));
    }
    if (!keep_dense) {
        if (!phi) return fail(OCN_EINVAL, "NULL pressure field");
        launch_copy_dense_to_field(g, phi, dist_dense_solution(s));
    }
    KERNEL_CHECK();
    return OCN_OK;
}
extern "C" int ocn_dist_poisson_backward_yz(ocn_dist_poisson_t s, double *phi) {
    NEED_INIT();
    if (!s || !s->recv || !phi) return fail(OCN_EINVAL, "solver / buffers not set");
    return dist_poisson_backward_yz(s, phi, false);
}
