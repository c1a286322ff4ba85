// ocn_implicit_z.h -- implicit_step! of ScalarDiffusivity(VerticallyImplicitTimeDiscretization(), ν, κ) with constant coefficients
// (TurbulenceClosures/vertically_implicit_diffusion_solver.jl:58-121,189-213): the real batched tridiagonal solve along z, in place on
// a haloed field, right-hand side = the field itself (Solvers/batched_tridiagonal_solver.jl:219-245). One column per lane, coalesced
// along x, over the (i, j) = (1..Nx, 1..Ny) columns `launch!(arch, grid, :xy, ...)` covers and the levels k = 1..Nz -- for Center and
// Face fields alike: column Nx + 1 of u on a Bounded x and level Nz + 1 of w are not part of the system.
#pragma once
#include "ocn_device.h"

// The three diagonals at the index the reference's functions are CALLED with. ZF: the field sits at z-Faces (w). `wall`: the column
// lies on a wall of its own staggered direction (u at i = 1 of a Bounded / RightConnected x, v at j = 1 likewise in y), where
// peripheral_node (Grids/inactive_node.jl:152-162) is true at every level. A Bool factor is Julia's strong zero: x * false = copysign(0, x).
__device__ __forceinline__ bool ivd_outside(const DGrid &g, int k) { return k < 1 || k > g.Nz; }     // inactive_cell along a Bounded z

// ivd_upper_diagonal (:58-66 Center, :87-94 Face)
template <bool ZF> __device__ __forceinline__ double ivd_upper(const DGrid &g, int k, double dt, double coef, bool wall) {
    if (ZF) {
        const double nu = ivd_outside(g, k) ? copysign(0.0, coef) : coef;                                   // νzᶜᶜᶜ(k) * !inactive_node(k, c, c, c)
        const double du = -dt * nu * (g.rdzc[k - 1 + g.Hz] * g.rdzf[k - 1 + g.Hz]);
        return (wall || ivd_outside(g, k)) ? copysign(0.0, du) : du;                                         // !peripheral_node(k, ℓx, ℓy, c)
    }
    const double kap = (ivd_outside(g, k + 1) && ivd_outside(g, k)) ? copysign(0.0, coef) : coef;             // κ(k+1) * !inactive_node(k+1, ℓx, ℓy, f)
    const double du = -dt * kap * (g.rdzc[k - 1 + g.Hz] * g.rdzf[k + g.Hz]);
    return (wall || ivd_outside(g, k + 1) || ivd_outside(g, k)) ? copysign(0.0, du) : du;                     // !peripheral_node(k+1, ℓx, ℓy, f)
}

// ivd_lower_diagonal (:68-79 Center, called with k′ and k = k′ + 1; :96-104 Face, called with k and k′ = k + 2 -- the shifts as written)
template <bool ZF> __device__ __forceinline__ double ivd_lower(const DGrid &g, int kc, double dt, double coef, bool wall) {
    if (ZF) {
        const int kp = kc + 2;
        const double nu = ivd_outside(g, kp - 1) ? copysign(0.0, coef) : coef;                              // ν(k′-1) * !inactive_node(k′-1, c, c, c)
        const double dl = -dt * nu * (g.rdzc[kp - 1 + g.Hz] * g.rdzf[kp - 2 + g.Hz]);                       // Δz⁻¹ᶜ(k′) Δz⁻¹ᶠ(k′-1)
        return (wall || ivd_outside(g, kc)) ? copysign(0.0, dl) : dl;                                        // !peripheral_node(k, ℓx, ℓy, c)
    }
    const int k = kc + 1;
    const double kap = (ivd_outside(g, k) && ivd_outside(g, k - 1)) ? copysign(0.0, coef) : coef;             // κ(k) * !inactive_node(k, ℓx, ℓy, f)
    const double dl = -dt * kap * (g.rdzc[k - 1 + g.Hz] * g.rdzf[k - 1 + g.Hz]);
    return (wall || ivd_outside(g, kc)) ? copysign(0.0, dl) : dl;                                            // !peripheral_node(k′, ℓx, ℓy, c)
}

// ivd_diagonal (:107-110): one - Δt * implicit_linear_coefficient (zero) - upper(k) - lower(k-1)
template <bool ZF> __device__ __forceinline__ double ivd_diagonal(const DGrid &g, int k, double dt, double coef, bool wall) {
    return ((1.0 - dt * 0.0) - ivd_upper<ZF>(g, k, dt, coef, wall)) - ivd_lower<ZF>(g, k - 1, dt, coef, wall);
}

#define OCN_IVD_GUARD (10.0 * 2.220446049250313e-16)        // abs(β) > 10 eps(Float64)
#define OCN_IVD_TB 8                                        // levels whose loads are issued together, ahead of the recurrence

// Every thread evaluates the loop of solve_batched_tridiagonal_system_z! for its column, scratch t in memory (dense,
// (i-1) + Nx ((j-1) + Ny (k-1))). fx / fy: the field sits at x- / y-Faces. The recurrences are serial in k, the loads are not: blocks of
// OCN_IVD_TB levels are fetched first, then swept (as tridiagonal_z_kernel does for the spectra). Two tuned forms -- a(k-1), β(k), t(k)
// and the guard from a per-level table formed by a one-thread launch, the column kept in place or in shared memory between the sweeps --
// returned the same bits but measured SLOWER (with 65 536 columns there is one wave per SIMD, the kernel waits on memory
// latency and the arithmetic it would save is hidden, while the table's serial recurrence is a launch of its own) and are not shipped.
template <bool ZF>
__global__ void __launch_bounds__(64) implicit_step_z_kernel(DGrid g, FView phi, double *__restrict__ t, double dt, double coef, bool fx, bool fy) {
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x;
    const int j = 1 + blockIdx.y;
    if (i > g.Nx || j > g.Ny) return;
    const bool wall = (fx && i == 1 && wall_lo(g.tx)) || (fy && j == 1 && wall_lo(g.ty));
    const int Nz = g.Nz;
    const long st = phi.s2, stt = (long)g.Nx * g.Ny;
    double *p = phi.p + phi.lin(i, j, 1);
    double *tq = t + (long)(i - 1) + (long)g.Nx * (j - 1);
    double beta = ivd_diagonal<ZF>(g, 1, dt, coef, wall);
    double prev = p[0] / beta;
    p[0] = prev;
    for (int k0 = 2; k0 <= Nz; k0 += OCN_IVD_TB) {
        double fb[OCN_IVD_TB];
#pragma unroll
        for (int n = 0; n < OCN_IVD_TB; ++n)
            if (k0 + n <= Nz) fb[n] = p[(long)(k0 + n - 1) * st];
#pragma unroll
        for (int n = 0; n < OCN_IVD_TB; ++n) {
            const int k = k0 + n;
            if (k <= Nz) {
                const double ck1 = ivd_upper<ZF>(g, k - 1, dt, coef, wall), bk = ivd_diagonal<ZF>(g, k, dt, coef, wall),
                             ak1 = ivd_lower<ZF>(g, k - 1, dt, coef, wall);
                const double tk = ck1 / beta;
                tq[(long)(k - 1) * stt] = tk;
                beta = bk - ak1 * tk;
                const double fk = fb[n];                    // the right-hand side is the field: f[k] and the untouched ϕ[k] are one value
                const bool dd = fabs(beta) > OCN_IVD_GUARD;
                const double star = (fk - ak1 * prev) / beta;
                prev = dd ? star : fk;
                p[(long)(k - 1) * st] = prev;
            }
        }
    }
    for (int k0 = Nz - 1; k0 >= 1; k0 -= OCN_IVD_TB) {
        double tb[OCN_IVD_TB], pb[OCN_IVD_TB];
#pragma unroll
        for (int n = 0; n < OCN_IVD_TB; ++n)
            if (k0 - n >= 1) { tb[n] = tq[(long)(k0 - n) * stt]; pb[n] = p[(long)(k0 - n - 1) * st]; }      // t[k+1], ϕ[k]
#pragma unroll
        for (int n = 0; n < OCN_IVD_TB; ++n) {
            const int k = k0 - n;
            if (k >= 1) {
                prev = pb[n] - tb[n] * prev;
                p[(long)(k - 1) * st] = prev;
            }
        }
    }
}
