// ocn_advect_split.h -- advection where the advecting velocities are not the advected field: the kernels behind background_fields
// (Models/NonhydrostaticModels/background_fields.jl, nonhydrostatic_tendency_kernel_functions.jl:86-94,148-156,213-221,276-293):
//
//     G_φ = - div(advection, U + Ū, φ) - div(advection, U, Φ̄) + ...
//
//   sum_parent_kernel          U + Ū over a whole parent array (SumOfArrays{2}, Utils/sum_of_arrays.jl:23,39-41: one IEEE addition per access)
//   advective_tendency_kernel  the per-field kernel of ocn_kernels.h with separate advecting views and an advected view, and a
//                              compile-time accumulate flag: every topology, Flat and reduced-order directions, launch ranges
//   role_split_kernel          the flux-sharing role kernel (ocn_tendency_roles.h) compiled with SPLIT: a launch names the advecting
//                              arrays, one advected array per role, the roles it evaluates, and may accumulate into the tendency
// Same IEEE operation sequence per flux as the kernels they generalise (mom_flux / tracer_flux, x_flux / y_flux / z_flux).
#pragma once
#include "ocn_kernels.h"
#include "ocn_tendency_roles.h"

__global__ void __launch_bounds__(256) sum_parent_kernel(const double *__restrict__ a, const double *__restrict__ b, double *__restrict__ out, long n) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += stride) out[q] = a[q] + b[q];
}

// div_𝐯u / div_𝐯v / div_𝐯w (Advection/momentum_advection_operators.jl:46-83) and div_Uc (tracer_advection_operators.jl:29-33) of the
// advected field psi (at the location of F) by the velocities (ua, va, wa). ACC false: G = -div + 0.0 (tendency_kernel); true: G = G - div.
template <int F, bool ACC>
__global__ void __launch_bounds__(256) advective_tendency_kernel(DGrid g, FView ua, FView va, FView wa, FView psi, FView G, Range6 r) {
    const int i = r.i0 + blockIdx.x * blockDim.x + threadIdx.x;
    const int j = r.j0 + blockIdx.y * blockDim.y + threadIdx.y;
    const int k = r.k0 + blockIdx.z;
    if (i > r.i1 || j > r.j1 || k > r.k1) return;
    double dx, dy, dz, vinv;
    if (F == F_U) {
        vinv = g.vinv_c[k - 1 + g.Hz];
        dx = mom_flux<AQ_U, 0, true, 0, true>(g, ua, psi, i, j, k) - mom_flux<AQ_U, 0, true, 0, true>(g, ua, psi, i - 1, j, k);
        dy = mom_flux<AQ_V, 0, false, 1, false>(g, va, psi, i, j + 1, k) - mom_flux<AQ_V, 0, false, 1, false>(g, va, psi, i, j, k);
        dz = mom_flux<AQ_W, 0, false, 2, false>(g, wa, psi, i, j, k + 1) - mom_flux<AQ_W, 0, false, 2, false>(g, wa, psi, i, j, k);
    } else if (F == F_V) {
        vinv = g.vinv_c[k - 1 + g.Hz];
        dx = mom_flux<AQ_U, 1, false, 0, false>(g, ua, psi, i + 1, j, k) - mom_flux<AQ_U, 1, false, 0, false>(g, ua, psi, i, j, k);
        dy = mom_flux<AQ_V, 1, true, 1, true>(g, va, psi, i, j, k) - mom_flux<AQ_V, 1, true, 1, true>(g, va, psi, i, j - 1, k);
        dz = mom_flux<AQ_W, 1, false, 2, false>(g, wa, psi, i, j, k + 1) - mom_flux<AQ_W, 1, false, 2, false>(g, wa, psi, i, j, k);
    } else if (F == F_W) {
        vinv = g.vinv_f[k - 1 + g.Hz];
        dx = mom_flux<AQ_U, 2, false, 0, false>(g, ua, psi, i + 1, j, k) - mom_flux<AQ_U, 2, false, 0, false>(g, ua, psi, i, j, k);
        dy = mom_flux<AQ_V, 2, false, 1, false>(g, va, psi, i, j + 1, k) - mom_flux<AQ_V, 2, false, 1, false>(g, va, psi, i, j, k);
        dz = mom_flux<AQ_W, 2, true, 2, true>(g, wa, psi, i, j, k) - mom_flux<AQ_W, 2, true, 2, true>(g, wa, psi, i, j, k - 1);
    } else {
        vinv = g.vinv_c[k - 1 + g.Hz];
        dx = tracer_flux<0>(g, ua, psi, i + 1, j, k) - tracer_flux<0>(g, ua, psi, i, j, k);
        dy = tracer_flux<1>(g, va, psi, i, j + 1, k) - tracer_flux<1>(g, va, psi, i, j, k);
        dz = tracer_flux<2>(g, wa, psi, i, j, k + 1) - tracer_flux<2>(g, wa, psi, i, j, k);
    }
    const double div = vinv * ((dx + dy) + dz);
    if (ACC) G.at(i, j, k) = G.at(i, j, k) - div;
    else     G.at(i, j, k) = -div + 0.0;
}

// ---- the role kernel with advecting != advected ----
// RoleArgs of the largest model (U[f]: the advected array of field f, G[f]: its tendency) + the advecting arrays + the fields this
// launch evaluates: a workgroup slot takes role[slot % nrole]
struct RoleSplitArgs : RoleArgs<OCN_MAX_FIELDS> {
    const double *A[3];
    int nrole;
    int role[OCN_MAX_FIELDS];
};

template <int TY, bool BZ, bool ACC>
__global__ void __launch_bounds__(64 * (TY + 1), OCN_ROLE_WAVES) role_split_kernel(DGrid gin, RoleSplitArgs a) {
    __shared__ double FX[2][TY][66];
    __shared__ double FY[2][TY + 1][64];

    DGrid g = gin;
    g.tx = 0; g.ty = 0; g.tz = BZ ? 1 : 0;

    // the same placement as role_tendency_kernel, over the nrole fields of this launch
    const unsigned d = blockIdx.x, xcd = d & 7u, slot = d >> 3, nr = (unsigned)a.nrole;
    const unsigned pair = xcd * (unsigned)a.band + slot / nr;
    if (slot / nr >= (unsigned)a.band || pair >= (unsigned)a.npair) return;
    const int fidx = a.role[slot % nr];
    const unsigned tile = pair % (unsigned)a.ntile, chunk = pair / (unsigned)a.ntile;
    const int i0 = a.r.i0 + (int)(tile % (unsigned)a.ntile_x) * 64, j0 = a.r.j0 + (int)(tile / (unsigned)a.ntile_x) * TY;
    const int kc0 = a.r.k0 + (int)chunk * a.kchunk;
    const int kc1 = min(kc0 + a.kchunk - 1, a.r.k1);
    if (fidx == 0) role_march<ROLE_U, TY, false, BZ, 0, false, RoleSplitArgs, true, ACC>(g, a, 0, i0, j0, kc0, kc1, FX, FY);
    else if (fidx == 1) role_march<ROLE_V, TY, false, BZ, 0, false, RoleSplitArgs, true, ACC>(g, a, 1, i0, j0, kc0, kc1, FX, FY);
    else if (fidx == 2) role_march<ROLE_W, TY, false, BZ, 0, false, RoleSplitArgs, true, ACC>(g, a, 2, i0, j0, kc0, kc1, FX, FY);
    else role_march<ROLE_C, TY, false, BZ, 0, false, RoleSplitArgs, true, ACC>(g, a, fidx, i0, j0, kc0, kc1, FX, FY);
}

// One launch: the fields `roles` (indices into psi / G: 0 u, 1 v, 2 w, 3.. tracers), advected by adv = (ua, va, wa). Reference arithmetic
// only (the caller checks: fused_tendency_supported, role_tendency_supported, arithmetic == 0). `range` as in launch_roles_n.
static inline int launch_role_split(const OcnOptions &o, const DGrid &g, hipStream_t stream, const double *const adv[3], const double *const *psi,
                                    double *const *G, const int *roles, int nrole, const int *range, bool accumulate) {
    if (nrole <= 0) return 0;
    if (nrole > OCN_MAX_FIELDS || o.arithmetic != 0) return -2;
    RoleSplitArgs a;
    for (int f = 0; f < OCN_MAX_FIELDS; ++f) { a.U[f] = nullptr; a.G[f] = nullptr; a.Un[f] = nullptr; a.Gm[f] = nullptr; a.role[f] = 0; }
    a.ftab = nullptr;
    for (int c = 0; c < 3; ++c) a.A[c] = adv[c];
    a.nrole = nrole;
    for (int q = 0; q < nrole; ++q) {
        const int f = roles[q];
        if (f < 0 || f >= OCN_MAX_FIELDS || !psi[f] || !G[f]) return -2;
        a.role[q] = f; a.U[f] = psi[f]; a.G[f] = G[f];
    }
    a.has_zeta = 0; a.store_G = 1; a.dt = 0.0; a.gamma = 0.0; a.zeta = 0.0;
    const int Px = g.Nx + 2 * g.Hx, Py = g.Ny + 2 * g.Hy;
    a.s1 = Px;
    a.s2 = (unsigned)((long)Px * Py);
    a.off = (g.Hx - 1) + (long)Px * (g.Hy - 1);
    if (range) {
        a.r = Range6{range[0], range[1], range[2], range[3], range[4], range[5]};
        a.wk0 = a.r.k0;
    } else {
        a.r = Range6{1, g.Nx, 1, g.Ny, 1, g.Nz};
        a.wk0 = (g.tz != 0 && g.Nz > 1) ? 2 : 1;
    }
    constexpr int TY = OCN_ROLE_TY;
    const int nx = a.r.i1 - a.r.i0 + 1, ny = a.r.j1 - a.r.j0 + 1, nz = a.r.k1 - a.r.k0 + 1;
    if (nx <= 0 || ny <= 0 || nz <= 0) return 0;
    a.ntile_x = (nx + 63) / 64;
    a.ntile = a.ntile_x * ((ny + TY - 1) / TY);
    a.kchunk = o.role_kchunk > 0 ? o.role_kchunk : pick_role_kchunk((long)a.ntile * nrole, nz);
    const int nchunk = (nz + a.kchunk - 1) / a.kchunk;
    a.npair = a.ntile * nchunk;
    a.band = (a.npair + 7) / 8;
    const unsigned nblocks = (unsigned)a.band * 8u * (unsigned)nrole;
    const dim3 blk(64 * (TY + 1));
#define OCN_LAUNCH_SPLIT(BZV, ACCV) hipLaunchKernelGGL((role_split_kernel<TY, BZV, ACCV>), dim3(nblocks), blk, (size_t)o.role_ldspad, stream, g, a)
    if (g.tz != 0) { if (accumulate) OCN_LAUNCH_SPLIT(true, true); else OCN_LAUNCH_SPLIT(true, false); }
    else           { if (accumulate) OCN_LAUNCH_SPLIT(false, true); else OCN_LAUNCH_SPLIT(false, false); }
#undef OCN_LAUNCH_SPLIT
    return 0;
}
