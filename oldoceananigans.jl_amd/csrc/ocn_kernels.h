// ocn_kernels.h -- HIP kernels of the hot path (reference kernel inventory: SURVEY.md 2.1). gfx950 / wave64.
// Families with a header of their own: the line FFTs (ocn_line_fft.h), the kernels around the pressure solve (ocn_pressure_step.h), the
// halo fills, the Flux-condition kernels and the halo buffers of partitioned runs (ocn_boundary_conditions.h), the turbulence closures
// (ocn_closures.h, included below where the tendency epilogues need it).
#pragma once
#include "ocn_device.h"
#include "ocn_immersed.h"
#include "ocn_line_fft.h"

// ---------------------------------------------------------------------------------------------------------------------
// advective fluxes (src/Advection/upwind_biased_advective_fluxes.jl:23-121), evaluated straight from global memory.
// This is the "as launched by the reference" formulation (each face flux evaluated by both adjacent cells); the fused
// flux-sharing kernel lives in ocn_tendency_fused.h.
// ---------------------------------------------------------------------------------------------------------------------
enum { AQ_U = 0, AQ_V = 1, AQ_W = 2 };

// area-weighted transports  Ax_qᶠᶜᶜ(u), Ay_qᶜᶠᶜ(v), Az_qᶜᶜᶠ(w)  (Operators/products_between_fields_and_grid_metrics.jl:5-14)
template <int AQ> __device__ __forceinline__ double area_q(const DGrid &g, const FView &f, int i, int j, int k) {
    double a = AQ == AQ_U ? g.ax[k - 1 + g.Hz] : (AQ == AQ_V ? g.ay[k - 1 + g.Hz] : g.az);
    return a * f.at(i, j, k);
}

// symmetric interpolation of a transport along D; CEN: ᶜ variant (stencil of face idx+1). B: buffer of the scheme of the
// direction the FLUX points along (adapt_advection_order; 3 unless that direction has fewer than 3 cells)
// IM: NoImm, or the ImmView of an immersed grid (ocn_immersed.h) -- the order entry then stands where outside_symmetric_halo stood
template <int AQ, int D, bool CEN, class IM = NoImm>
__device__ __forceinline__ double sym_transport(const DGrid &g, const FView &f, int i, int j, int k, int B, const IM &im = IM()) {
    // interpolation along a Flat direction is the identity (flat_advective_fluxes.jl:35-50)
    if ((D == 0 ? g.tx : (D == 1 ? g.ty : g.tz)) == OCN_FLAT) return area_q<AQ>(g, f, i, j, k);
    const int idx = D == 0 ? i : (D == 1 ? j : k);
    const int o = CEN ? 1 : 0;
    double q[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        int m = o - 2 + n;
        if (B < 3 && (n == 0 || n == 3)) { q[n] = 0.0; continue; }      // Centered(order = 2): two points, one halo cell
        q[n] = D == 0 ? area_q<AQ>(g, f, i + m, j, k) : (D == 1 ? area_q<AQ>(g, f, i, j + m, k) : area_q<AQ>(g, f, i, j, k + m));
    }
    if (B < 3) return symmetric_interp_low(q[1], q[2]);
    if constexpr (IM::on) return symmetric_interp_order(q[0], q[1], q[2], q[3], im.template order<D, CEN>(i, j, k));
    const int T = D == 0 ? g.tx : (D == 1 ? g.ty : g.tz);
    const bool lo = wall_lo(T), hi = wall_hi(T);
    const int N = D == 0 ? g.Nx : (D == 1 ? g.Ny : g.Nz);
    return symmetric_interp(q[0], q[1], q[2], q[3], lo | hi, idx, CEN, N, lo, hi);
}

template <int D, bool CEN, class IM = NoImm>
__device__ __forceinline__ double biased_field(const DGrid &g, const FView &c, bool left, int i, int j, int k, const IM &im = IM()) {
    const int idx = D == 0 ? i : (D == 1 ? j : k);
    const int o = CEN ? 1 : 0;
    const long st = c.stride<D>();
    const double *p = c.p + c.lin(i, j, k) + (o - 3) * st;
    const int T = D == 0 ? g.tx : (D == 1 ? g.ty : g.tz);
    const bool lo = wall_lo(T), hi = wall_hi(T), bounded = lo | hi;
    const int N = D == 0 ? g.Nx : (D == 1 ? g.Ny : g.Nz);
    const int B = D == 0 ? g.Bx : (D == 1 ? g.By : g.Bz);
    if (B < 3) {                                                         // reduced scheme: the halo may be only B cells deep
        const double s2 = p[2 * st], s3 = p[3 * st];
        const double s1 = B == 2 ? p[st] : 0.0, s4 = B == 2 ? p[4 * st] : 0.0;
        if constexpr (IM::on) return biased_interp_order(0.0, s1, s2, s3, s4, 0.0, left, min(B, im.template order<D, CEN>(i, j, k)));
        return biased_interp_low(s1, s2, s3, s4, left, bounded, idx, CEN, N, B, lo, hi);
    }
    double s0 = p[0], s1 = p[st], s2 = p[2 * st], s3 = p[3 * st], s4 = p[4 * st], s5 = p[5 * st];
    if constexpr (IM::on) return biased_interp_order(s0, s1, s2, s3, s4, s5, left, im.template order<D, CEN>(i, j, k));
    return biased_interp(s0, s1, s2, s3, s4, s5, left, bounded, idx, CEN, N, lo, hi);
}

// advective_momentum_flux_{U,V,W}{u,v,w}: transport AQ interpolated along DS (CS), advected field reconstructed along
// DB (CB).
// On an immersed grid the flux is conditional_flux_{ccc,ffc,fcf,cff}(i, j, k, ibg, 0, flux) (immersed_advective_fluxes.jl:39-55).
template <int AQ, int DS, bool CS, int DB, bool CB, class IM = NoImm>
__device__ __forceinline__ double mom_flux(const DGrid &g, const FView &adv, const FView &psi, int i, int j, int k, const IM &im = IM()) {
    if ((DB == 0 ? g.tx : (DB == 1 ? g.ty : g.tz)) == OCN_FLAT) return 0.0;     // fluxes along a Flat direction vanish (:13-27)
    double ut = sym_transport<AQ, DS, CS, IM>(g, adv, i, j, k, DB == 0 ? g.Bx : (DB == 1 ? g.By : g.Bz), im);
    double pr = biased_field<DB, CB, IM>(g, psi, ut > 0, i, j, k, im);
    if constexpr (IM::on) return im.flux(imm_momentum_flux_bit<DS, DB>(), i, j, k, ut * pr);
    return ut * pr;
}

// advective_tracer_flux_{x,y,z} (:99-121): A * U[i,j,k] * cR
// (on an immersed grid conditional_flux_{fcc,cfc,ccf}, immersed_advective_fluxes.jl:57-59)
template <int D, class IM = NoImm>
__device__ __forceinline__ double tracer_flux(const DGrid &g, const FView &vel, const FView &c, int i, int j, int k, const IM &im = IM()) {
    if ((D == 0 ? g.tx : (D == 1 ? g.ty : g.tz)) == OCN_FLAT) return 0.0;
    double ut = vel.at(i, j, k);
    double cr = biased_field<D, false, IM>(g, c, ut > 0, i, j, k, im);
    double a = D == 0 ? g.ax[k - 1 + g.Hz] : (D == 1 ? g.ay[k - 1 + g.Hz] : g.az);
    if constexpr (IM::on) return im.flux(IMM_FCC + D, i, j, k, a * ut * cr);
    return a * ut * cr;
}

enum { F_U = 0, F_V = 1, F_W = 2, F_C = 3 };

// compute_Gu!/Gv!/Gw!/Gc! (Models/NonhydrostaticModels/compute_nonhydrostatic_tendencies.jl:138-163) with
// div_𝐯u/v/w (Advection/momentum_advection_operators.jl:46-83) and div_Uc (tracer_advection_operators.jl:29-33).
template <int F>
__global__ void __launch_bounds__(256) tendency_kernel(DGrid g, FView u, FView v, FView w, FView c, FView G, Range6 r) {
    const int i = r.i0 + blockIdx.x * blockDim.x + threadIdx.x;
    const int j = r.j0 + blockIdx.y * blockDim.y + threadIdx.y;
    const int k = r.k0 + blockIdx.z;
    if (i > r.i1 || j > r.j1 || k > r.k1) return;
    double dx, dy, dz, vinv;
    if (F == F_U) {
        vinv = g.vinv_c[k - 1 + g.Hz];
        dx = mom_flux<AQ_U, 0, true, 0, true>(g, u, u, i, j, k) - mom_flux<AQ_U, 0, true, 0, true>(g, u, u, i - 1, j, k);
        dy = mom_flux<AQ_V, 0, false, 1, false>(g, v, u, i, j + 1, k) - mom_flux<AQ_V, 0, false, 1, false>(g, v, u, i, j, k);
        dz = mom_flux<AQ_W, 0, false, 2, false>(g, w, u, i, j, k + 1) - mom_flux<AQ_W, 0, false, 2, false>(g, w, u, i, j, k);
    } else if (F == F_V) {
        vinv = g.vinv_c[k - 1 + g.Hz];
        dx = mom_flux<AQ_U, 1, false, 0, false>(g, u, v, i + 1, j, k) - mom_flux<AQ_U, 1, false, 0, false>(g, u, v, i, j, k);
        dy = mom_flux<AQ_V, 1, true, 1, true>(g, v, v, i, j, k) - mom_flux<AQ_V, 1, true, 1, true>(g, v, v, i, j - 1, k);
        dz = mom_flux<AQ_W, 1, false, 2, false>(g, w, v, i, j, k + 1) - mom_flux<AQ_W, 1, false, 2, false>(g, w, v, i, j, k);
    } else if (F == F_W) {
        vinv = g.vinv_f[k - 1 + g.Hz];
        dx = mom_flux<AQ_U, 2, false, 0, false>(g, u, w, i + 1, j, k) - mom_flux<AQ_U, 2, false, 0, false>(g, u, w, i, j, k);
        dy = mom_flux<AQ_V, 2, false, 1, false>(g, v, w, i, j + 1, k) - mom_flux<AQ_V, 2, false, 1, false>(g, v, w, i, j, k);
        dz = mom_flux<AQ_W, 2, true, 2, true>(g, w, w, i, j, k) - mom_flux<AQ_W, 2, true, 2, true>(g, w, w, i, j, k - 1);
    } else {
        vinv = g.vinv_c[k - 1 + g.Hz];
        dx = tracer_flux<0>(g, u, c, i + 1, j, k) - tracer_flux<0>(g, u, c, i, j, k);
        dy = tracer_flux<1>(g, v, c, i, j + 1, k) - tracer_flux<1>(g, v, c, i, j, k);
        dz = tracer_flux<2>(g, w, c, i, j, k + 1) - tracer_flux<2>(g, w, c, i, j, k);
    }
    double div = vinv * ((dx + dy) + dz);
    G.at(i, j, k) = -div + 0.0;   // `-div - 0 + 0 ...` of the tendency functions: only maps -0.0 to +0.0
}

// The immersed instantiation (ocn_immersed.h), with the advecting velocities apart from the advected field like advective_tendency_kernel
// (ocn_advect_split.h): compute_Gu!/Gv!/Gw!/Gc! pass psi = u, v, w, c. Every cell of the launch range is written, immersed cells
// included -- the reference launches without an active-cells map.
template <int F, bool ACC>
__global__ void __launch_bounds__(256) immersed_tendency_kernel(DGrid g, ImmView im, FView ua, FView va, FView wa, FView psi, FView G, Range6 r) {
    const int i = r.i0 + blockIdx.x * blockDim.x + threadIdx.x;
    const int j = r.j0 + blockIdx.y * blockDim.y + threadIdx.y;
    const int k = r.k0 + blockIdx.z;
    if (i > r.i1 || j > r.j1 || k > r.k1) return;
    using IM = ImmView;
    double dx, dy, dz, vinv;
    if (F == F_U) {
        vinv = g.vinv_c[k - 1 + g.Hz];
        dx = mom_flux<AQ_U, 0, true, 0, true, IM>(g, ua, psi, i, j, k, im) - mom_flux<AQ_U, 0, true, 0, true, IM>(g, ua, psi, i - 1, j, k, im);
        dy = mom_flux<AQ_V, 0, false, 1, false, IM>(g, va, psi, i, j + 1, k, im) - mom_flux<AQ_V, 0, false, 1, false, IM>(g, va, psi, i, j, k, im);
        dz = mom_flux<AQ_W, 0, false, 2, false, IM>(g, wa, psi, i, j, k + 1, im) - mom_flux<AQ_W, 0, false, 2, false, IM>(g, wa, psi, i, j, k, im);
    } else if (F == F_V) {
        vinv = g.vinv_c[k - 1 + g.Hz];
        dx = mom_flux<AQ_U, 1, false, 0, false, IM>(g, ua, psi, i + 1, j, k, im) - mom_flux<AQ_U, 1, false, 0, false, IM>(g, ua, psi, i, j, k, im);
        dy = mom_flux<AQ_V, 1, true, 1, true, IM>(g, va, psi, i, j, k, im) - mom_flux<AQ_V, 1, true, 1, true, IM>(g, va, psi, i, j - 1, k, im);
        dz = mom_flux<AQ_W, 1, false, 2, false, IM>(g, wa, psi, i, j, k + 1, im) - mom_flux<AQ_W, 1, false, 2, false, IM>(g, wa, psi, i, j, k, im);
    } else if (F == F_W) {
        vinv = g.vinv_f[k - 1 + g.Hz];
        dx = mom_flux<AQ_U, 2, false, 0, false, IM>(g, ua, psi, i + 1, j, k, im) - mom_flux<AQ_U, 2, false, 0, false, IM>(g, ua, psi, i, j, k, im);
        dy = mom_flux<AQ_V, 2, false, 1, false, IM>(g, va, psi, i, j + 1, k, im) - mom_flux<AQ_V, 2, false, 1, false, IM>(g, va, psi, i, j, k, im);
        dz = mom_flux<AQ_W, 2, true, 2, true, IM>(g, wa, psi, i, j, k, im) - mom_flux<AQ_W, 2, true, 2, true, IM>(g, wa, psi, i, j, k - 1, im);
    } else {
        vinv = g.vinv_c[k - 1 + g.Hz];
        dx = tracer_flux<0, IM>(g, ua, psi, i + 1, j, k, im) - tracer_flux<0, IM>(g, ua, psi, i, j, k, im);
        dy = tracer_flux<1, IM>(g, va, psi, i, j + 1, k, im) - tracer_flux<1, IM>(g, va, psi, i, j, k, im);
        dz = tracer_flux<2, IM>(g, wa, psi, i, j, k + 1, im) - tracer_flux<2, IM>(g, wa, psi, i, j, k, im);
    }
    const double div = vinv * ((dx + dy) + dz);
    if (ACC) G.at(i, j, k) = G.at(i, j, k) - div;
    else     G.at(i, j, k) = -div + 0.0;
}

#include "ocn_closures.h"      // the turbulence closures (uses F_U .. F_C above; the tendency epilogues below call its closure_divergence)

// ---------------------------------------------------------------------------------------------------------------------
// Buoyancy: BuoyancyTracer | SeawaterBuoyancy(LinearEquationOfState), gravity along -z.
// _update_hydrostatic_pressure! (Models/NonhydrostaticModels/update_hydrostatic_pressure.jl:12-22) over i = 0:Nx+1, j = 0:Ny+1
// (:43-50): pHY′[Nz] = -z_dot_g_b(Nz+1) Δzᶠ(Nz+1); pHY′[k] = pHY′[k+1] - z_dot_g_b(k+1) Δzᶠ(k+1), z_dot_g_bᶜᶜᶠ = 1 * ℑzᵃᵃᶠ(b)
// (BuoyancyFormulations/g_dot_b.jl:4). One thread per column, coalesced in x.
// ---------------------------------------------------------------------------------------------------------------------
struct BuoyancyArgs {
    int kind;                 // 1: tracer b; 2: g (α T - β S) (linear_equation_of_state.jl:71-73)
    const double *bT, *S;
    double grav, alpha, beta;
};
// ... and ĝ_z = -gravity_unit_vector[3] (buoyancy_force.jl:54) for the TILT instantiations of hydrostatic_pressure_kernel: a type of its
// own, so that the arguments of the others stay what they were
struct TiltedBuoyancyArgs : BuoyancyArgs {
    double ghat_z;
};
template <bool TILT> struct HydrostaticArgs { typedef BuoyancyArgs type; };
template <> struct HydrostaticArgs<true> { typedef TiltedBuoyancyArgs type; };
__device__ __forceinline__ double buoyancy_perturbation(const BuoyancyArgs &B, long q) {
    return B.kind == 1 ? B.bT[q] : B.grav * (B.alpha * B.bT[q] - B.beta * B.S[q]);
}

#ifndef OCN_HYDRO_TB
#define OCN_HYDRO_TB 32
#endif
// KIND (BuoyancyArgs::kind) is compile-time and the levels of a batch are clamped instead of guarded, so that the 2 * TB loads of a batch are
// straight-line code: with the run-time `kind` test and the `k >= 1` guard around each load the compiler waited for every level's pair before
// issuing the next (one memory round trip per level: 0.098 ms at 256 x 256 x 128, one wave per SIMD, nothing to hide it behind).
// TILT: BuoyancyForce(formulation; gravity_unit_vector) -- z_dot_g_bᶜᶜᶠ = ĝ_z * ℑzᵃᵃᶠ(b) (g_dot_b.jl:4) with ĝ_z from the arguments in
// place of the literal 1 of NegativeZDirection (buoyancy_force.jl:54,58); compile-time, so the KIND-only instantiations keep their code.
template <int KIND, bool TILT = false>
__global__ void __launch_bounds__(256) hydrostatic_pressure_kernel(DGrid g, FView c, typename HydrostaticArgs<TILT>::type B, double *pHY, int i0, int i1, int j0, int j1) {
    const int i = i0 + blockIdx.x * blockDim.x + threadIdx.x;
    const int j = j0 + blockIdx.y * blockDim.y + threadIdx.y;
    if (i > i1 || j > j1) return;
    const int Nz = g.Nz;
    const long q1 = c.lin(i, j, 1);                                     // level k at q1 + (k - 1) s2
    auto b_of = [&](double t, double s) { return KIND == 1 ? t : B.grav * (B.alpha * t - B.beta * s); };
    double bk1 = b_of(B.bT[q1 + (long)Nz * c.s2], KIND == 1 ? 0.0 : B.S[q1 + (long)Nz * c.s2]);          // b[Nz + 1]
    double p = 0.0;
    // the recurrence is serial in k but its loads are not: fetch TB levels, then sweep them (few columns => latency-bound otherwise:
    // 66 K columns at 256 x 256 are one wave per SIMD)
    constexpr int TB = OCN_HYDRO_TB;
    for (int k0 = Nz; k0 >= 1; k0 -= TB) {
        double tb[TB], sb[TB];
#pragma unroll
        for (int n = 0; n < TB; ++n) {
            const long q = q1 + (long)(max(k0 - n, 1) - 1) * c.s2;      // below the bottom: level 1 again (in bounds, unused)
            tb[n] = B.bT[q];
            sb[n] = KIND == 1 ? 0.0 : B.S[q];
        }
#pragma unroll
        for (int n = 0; n < TB; ++n) {
            const int k = k0 - n;
            if (k >= 1) {
                const double bk = b_of(tb[n], sb[n]);
                double zb;
                if constexpr (TILT) zb = B.ghat_z * (0.5 * (bk + bk1));
                else                zb = 1 * (0.5 * (bk + bk1));
                const double dzf = g.dzf[k + g.Hz];            // Δzᶠ(k+1)
                p = k == Nz ? -zb * dzf : p - zb * dzf;
                pHY[q1 + (long)(k - 1) * c.s2] = p;
                bk1 = bk;
            }
        }
    }
}

// G_u -= ∂xᶠᶜᶜ pHY′, G_v -= ∂yᶜᶠᶜ pHY′ (nonhydrostatic_tendency_kernel_functions.jl:14-19,97,159) on tendencies holding the
// advective part; ranges = the tendency ranges of u and v
__device__ __forceinline__ double hydrostatic_gradient_x(const DGrid &g, const FView &p, int i, int j, int k) {
    return g.tx == OCN_FLAT ? 0.0 : (p.at(i, j, k) - p.at(i - 1, j, k)) * g.rdx;
}
__device__ __forceinline__ double hydrostatic_gradient_y(const DGrid &g, const FView &p, int i, int j, int k) {
    return g.ty == OCN_FLAT ? 0.0 : (p.at(i, j, k) - p.at(i, j - 1, k)) * g.rdy;
}

__global__ void __launch_bounds__(256) hydrostatic_gradient_kernel(DGrid g, FView p, FView Gu, FView Gv, Range6 ru, Range6 rv) {
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x;
    const int j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    const int k = 1 + blockIdx.z;
    if (i > g.Nx || j > g.Ny || k > g.Nz) return;
    if (i >= ru.i0 && i <= ru.i1 && j >= ru.j0 && j <= ru.j1 && k >= ru.k0 && k <= ru.k1)
        Gu.at(i, j, k) = Gu.at(i, j, k) - hydrostatic_gradient_x(g, p, i, j, k);
    if (i >= rv.i0 && i <= rv.i1 && j >= rv.j0 && j <= rv.j1 && k >= rv.k0 && k <= rv.k1)
        Gv.at(i, j, k) = Gv.at(i, j, k) - hydrostatic_gradient_y(g, p, i, j, k);
}

// ---------------------------------------------------------------------------------------------------------------------
// coriolis = FPlane(f) (Coriolis/f_plane.jl:48-52): x_f_cross_U = -f active_weighted_ℑxyᶠᶜᶜ(v), y_f_cross_U =
// f active_weighted_ℑxyᶜᶠᶜ(u). The active-weighted average (Operators/interpolation_operators.jl:116-130) divides the four-point
// average by the fraction of non-peripheral nodes (Grids/inactive_node.jl:152-156). G_u -= x_f_cross_U, G_v -= y_f_cross_U on
// tendencies holding the advective part.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool inactive_cell(const DGrid &g, int i, int j, int k) {
    return ((wall_lo(g.tx) && i < 1) || (wall_hi(g.tx) && i > g.Nx)) || ((wall_lo(g.ty) && j < 1) || (wall_hi(g.ty) && j > g.Ny)) ||
           (g.tz == OCN_BOUNDED && (k < 1 || k > g.Nz));
}

// (x_f_cross_U_with / y_f_cross_U_with below are the same two bodies with the inactive-cell test handed in, for immersed grids: a change
// here is a change there.)
// x_f_cross_U at (f, c, c) and y_f_cross_U at (c, f, c). The field is read through `q(di, dj)` = value at (i + di, j + dj, k): from memory
// (the stand-alone kernels) or from the registers of the marching epilogue -- one body for both, so the same operations on the same values.
template <class Q>
__device__ __forceinline__ double x_f_cross_U_of(const DGrid &g, double f, Q q, int i, int j, int k) {
    const bool fx = g.tx == OCN_FLAT, fy = g.ty == OCN_FLAT;
    // ℑxyᶠᶜᵃ = ℑyᵃᶜᵃ(ℑxᶠᵃᵃ ·): X(jj) = 0.5 (q[i-1, jj] + q[i, jj]); 0.5 (X(j) + X(j+1)); not_peripheral at (c, f, c)
    auto np = [&](int ii, int jj) { return !(inactive_cell(g, ii, jj, k) || inactive_cell(g, ii, jj - 1, k)) ? 1.0 : 0.0; };
    auto Xq = [&](int dj) { return fx ? q(0, dj) : 0.5 * (q(-1, dj) + q(0, dj)); };
    auto Xn = [&](int jj) { return fx ? np(i, jj) : 0.5 * (np(i - 1, jj) + np(i, jj)); };
    const double qa = fy ? Xq(0) : 0.5 * (Xq(0) + Xq(1));
    const double an = fy ? Xn(j) : 0.5 * (Xn(j) + Xn(j + 1));
    const double aw = an == 0 ? 0.0 : qa / an;
    return -f * aw;
}
template <class Q>
__device__ __forceinline__ double y_f_cross_U_of(const DGrid &g, double f, Q q, int i, int j, int k) {
    const bool fx = g.tx == OCN_FLAT, fy = g.ty == OCN_FLAT;
    // ℑxyᶜᶠᵃ = ℑyᵃᶠᵃ(ℑxᶜᵃᵃ ·): X(jj) = 0.5 (q[i, jj] + q[i+1, jj]); 0.5 (X(j-1) + X(j)); not_peripheral at (f, c, c)
    auto np = [&](int ii, int jj) { return !(inactive_cell(g, ii, jj, k) || inactive_cell(g, ii - 1, jj, k)) ? 1.0 : 0.0; };
    auto Xq = [&](int dj) { return fx ? q(0, dj) : 0.5 * (q(0, dj) + q(1, dj)); };
    auto Xn = [&](int jj) { return fx ? np(i, jj) : 0.5 * (np(i, jj) + np(i + 1, jj)); };
    const double qa = fy ? Xq(0) : 0.5 * (Xq(-1) + Xq(0));
    const double an = fy ? Xn(j) : 0.5 * (Xn(j - 1) + Xn(j));
    const double aw = an == 0 ? 0.0 : qa / an;
    return f * aw;
}
// The same two averages with inactive_cell at level k handed in as `inactive(ii, jj)`: bit 0 of the periphery byte on an immersed grid, whose
// peripheral_node counts the immersed cells (immersed_boundary_interface.jl:49). (Bodies apart from the ones above: those are part of the
// marching epilogue's instantiations, which keep their registers.)
template <class Q, class IC>
__device__ __forceinline__ double x_f_cross_U_with(const DGrid &g, double f, Q q, int i, int j, int k, IC inactive) {
    const bool fx = g.tx == OCN_FLAT, fy = g.ty == OCN_FLAT;
    // ℑxyᶠᶜᵃ = ℑyᵃᶜᵃ(ℑxᶠᵃᵃ ·): X(jj) = 0.5 (q[i-1, jj] + q[i, jj]); 0.5 (X(j) + X(j+1)); not_peripheral at (c, f, c)
    auto np = [&](int ii, int jj) { return !(inactive(ii, jj) || inactive(ii, jj - 1)) ? 1.0 : 0.0; };
    auto Xq = [&](int dj) { return fx ? q(0, dj) : 0.5 * (q(-1, dj) + q(0, dj)); };
    auto Xn = [&](int jj) { return fx ? np(i, jj) : 0.5 * (np(i - 1, jj) + np(i, jj)); };
    const double qa = fy ? Xq(0) : 0.5 * (Xq(0) + Xq(1));
    const double an = fy ? Xn(j) : 0.5 * (Xn(j) + Xn(j + 1));
    const double aw = an == 0 ? 0.0 : qa / an;
    return -f * aw;
}
template <class Q, class IC>
__device__ __forceinline__ double y_f_cross_U_with(const DGrid &g, double f, Q q, int i, int j, int k, IC inactive) {
    const bool fx = g.tx == OCN_FLAT, fy = g.ty == OCN_FLAT;
    // ℑxyᶜᶠᵃ = ℑyᵃᶠᵃ(ℑxᶜᵃᵃ ·): X(jj) = 0.5 (q[i, jj] + q[i+1, jj]); 0.5 (X(j-1) + X(j)); not_peripheral at (f, c, c)
    auto np = [&](int ii, int jj) { return !(inactive(ii, jj) || inactive(ii - 1, jj)) ? 1.0 : 0.0; };
    auto Xq = [&](int dj) { return fx ? q(0, dj) : 0.5 * (q(0, dj) + q(1, dj)); };
    auto Xn = [&](int jj) { return fx ? np(i, jj) : 0.5 * (np(i, jj) + np(i + 1, jj)); };
    const double qa = fy ? Xq(0) : 0.5 * (Xq(-1) + Xq(0));
    const double an = fy ? Xn(j) : 0.5 * (Xn(j - 1) + Xn(j));
    const double aw = an == 0 ? 0.0 : qa / an;
    return f * aw;
}
__device__ __forceinline__ double x_f_cross_U(const DGrid &g, double f, const FView &v, int i, int j, int k) {
    return x_f_cross_U_of(g, f, [&](int di, int dj) { return v.at(i + di, j + dj, k); }, i, j, k);
}
__device__ __forceinline__ double y_f_cross_U(const DGrid &g, double f, const FView &u, int i, int j, int k) {
    return y_f_cross_U_of(g, f, [&](int di, int dj) { return u.at(i + di, j + dj, k); }, i, j, k);
}

__global__ void __launch_bounds__(256) fplane_coriolis_kernel(DGrid g, double f, FView u, FView v, FView Gu, FView Gv, Range6 ru, Range6 rv) {
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x;
    const int j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    const int k = 1 + blockIdx.z;
    if (i > g.Nx || j > g.Ny || k > g.Nz) return;
    if (i >= ru.i0 && i <= ru.i1 && j >= ru.j0 && j <= ru.j1 && k >= ru.k0 && k <= ru.k1)
        Gu.at(i, j, k) = Gu.at(i, j, k) - x_f_cross_U(g, f, v, i, j, k);
    if (i >= rv.i0 && i <= rv.i1 && j >= rv.j0 && j <= rv.j1 && k >= rv.k0 && k <= rv.k1)
        Gv.at(i, j, k) = Gv.at(i, j, k) - y_f_cross_U(g, f, u, i, j, k);
}

// the same on an immersed grid: not_peripheral read from the periphery byte (ocn_immersed.h)
__global__ void __launch_bounds__(256) immersed_fplane_coriolis_kernel(DGrid g, ImmView im, double f, FView u, FView v, FView Gu, FView Gv, Range6 ru,
                                                                       Range6 rv) {
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x;
    const int j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    const int k = 1 + blockIdx.z;
    if (i > g.Nx || j > g.Ny || k > g.Nz) return;
    auto inactive = [&](int ii, int jj) { return im.bit(IMM_INACTIVE, ii, jj, k); };
    if (i >= ru.i0 && i <= ru.i1 && j >= ru.j0 && j <= ru.j1 && k >= ru.k0 && k <= ru.k1)
        Gu.at(i, j, k) = Gu.at(i, j, k) - x_f_cross_U_with(g, f, [&](int di, int dj) { return v.at(i + di, j + dj, k); }, i, j, k, inactive);
    if (i >= rv.i0 && i <= rv.i1 && j >= rv.j0 && j <= rv.j1 && k >= rv.k0 && k <= rv.k1)
        Gv.at(i, j, k) = Gv.at(i, j, k) - y_f_cross_U_with(g, f, [&](int di, int dj) { return u.at(i + di, j + dj, k); }, i, j, k, inactive);
}

// ---------------------------------------------------------------------------------------------------------------------
// coriolis = ConstantCartesianCoriolis(fx, fy, fz) (Coriolis/constant_cartesian_coriolis.jl:70-81): a constant rotation vector with all
// three components. x_f_cross_U = ℑxᶠᵃᵃ(fʸ ℑzᵃᵃᶜ(w) - fᶻ ℑyᵃᶜᵃ(v)), y_f_cross_U = ℑyᵃᶠᵃ(fᶻ ℑxᶜᵃᵃ(u) - fˣ ℑzᵃᵃᶜ(w)), z_f_cross_U =
// ℑzᵃᵃᶠ(fˣ ℑyᵃᶜᵃ(v) - fʸ ℑxᶜᵃᵃ(u)): plain two-point averages (no active weighting, no wall logic); an interpolation along a Flat
// direction is the identity (Operators/interpolation_operators.jl:87-112). The velocities are read through accessors
// q(di, dj, dk) = value at (i + di, j + dj, k + dk), never called with an offset along a Flat direction: one body for the stand-alone
// kernel and the epilogue.
// ---------------------------------------------------------------------------------------------------------------------
template <class QV, class QW>
__device__ __forceinline__ double x_f_cross_U_cartesian(const DGrid &g, double fy, double fz, QV v, QW w) {
    const bool flx = g.tx == OCN_FLAT, fly = g.ty == OCN_FLAT, flz = g.tz == OCN_FLAT;
    auto A = [&](int di) {                                   // fʸw_minus_fᶻv at (c, c, c) (:70-71)
        const double wz = flz ? w(di, 0, 0) : 0.5 * (w(di, 0, 0) + w(di, 0, 1));
        const double vy = fly ? v(di, 0, 0) : 0.5 * (v(di, 0, 0) + v(di, 1, 0));
        return fy * wz - fz * vy;
    };
    return flx ? A(0) : 0.5 * (A(-1) + A(0));                // ℑxᶠᵃᵃ (:79)
}
template <class QU, class QW>
__device__ __forceinline__ double y_f_cross_U_cartesian(const DGrid &g, double fx, double fz, QU u, QW w) {
    const bool flx = g.tx == OCN_FLAT, fly = g.ty == OCN_FLAT, flz = g.tz == OCN_FLAT;
    auto B = [&](int dj) {                                   // fᶻu_minus_fˣw at (c, c, c) (:73-74)
        const double ux = flx ? u(0, dj, 0) : 0.5 * (u(0, dj, 0) + u(1, dj, 0));
        const double wz = flz ? w(0, dj, 0) : 0.5 * (w(0, dj, 0) + w(0, dj, 1));
        return fz * ux - fx * wz;
    };
    return fly ? B(0) : 0.5 * (B(-1) + B(0));                // ℑyᵃᶠᵃ (:80)
}
template <class QU, class QV>
__device__ __forceinline__ double z_f_cross_U_cartesian(const DGrid &g, double fx, double fy, QU u, QV v) {
    const bool flx = g.tx == OCN_FLAT, fly = g.ty == OCN_FLAT, flz = g.tz == OCN_FLAT;
    auto C = [&](int dk) {                                   // fˣv_minus_fʸu at (c, c, c) (:76-77)
        const double vy = fly ? v(0, 0, dk) : 0.5 * (v(0, 0, dk) + v(0, 1, dk));
        const double ux = flx ? u(0, 0, dk) : 0.5 * (u(0, 0, dk) + u(1, 0, dk));
        return fx * vy - fy * ux;
    };
    return flz ? C(0) : 0.5 * (C(-1) + C(0));                // ℑzᵃᵃᶠ (:81)
}

// G_u -= x_f_cross_U, G_v -= y_f_cross_U, G_w -= z_f_cross_U on tendencies holding the advective part; each over its own range
__global__ void __launch_bounds__(256) cartesian_coriolis_kernel(DGrid g, double fx, double fy, double fz, FView u, FView v, FView w, FView Gu,
                                                                 FView Gv, FView Gw, Range6 ru, Range6 rv, Range6 rw) {
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x;
    const int j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    const int k = 1 + blockIdx.z;
    if (i > g.Nx || j > g.Ny || k > g.Nz) return;
    auto qu = [&](int di, int dj, int dk) { return u.at(i + di, j + dj, k + dk); };
    auto qv = [&](int di, int dj, int dk) { return v.at(i + di, j + dj, k + dk); };
    auto qw = [&](int di, int dj, int dk) { return w.at(i + di, j + dj, k + dk); };
    if (i >= ru.i0 && i <= ru.i1 && j >= ru.j0 && j <= ru.j1 && k >= ru.k0 && k <= ru.k1)
        Gu.at(i, j, k) = Gu.at(i, j, k) - x_f_cross_U_cartesian(g, fy, fz, qv, qw);
    if (i >= rv.i0 && i <= rv.i1 && j >= rv.j0 && j <= rv.j1 && k >= rv.k0 && k <= rv.k1)
        Gv.at(i, j, k) = Gv.at(i, j, k) - y_f_cross_U_cartesian(g, fx, fz, qu, qw);
    if (i >= rw.i0 && i <= rw.i1 && j >= rw.j0 && j <= rw.j1 && k >= rw.k0 && k <= rw.k1)
        Gw.at(i, j, k) = Gw.at(i, j, k) - z_f_cross_U_cartesian(g, fx, fy, qu, qv);
}

// ---------------------------------------------------------------------------------------------------------------------
// buoyancy = BuoyancyForce(formulation; gravity_unit_vector) (BuoyancyFormulations/buoyancy_force.jl:47-54, g_dot_b.jl:2-3):
// x_dot_g_bᶠᶜᶜ = ĝ_x ℑxᶠᵃᵃ(b), y_dot_g_bᶜᶠᶜ = ĝ_y ℑyᵃᶠᵃ(b) with ĝ = -gravity_unit_vector and b the buoyancy perturbation at (c, c, c),
// read through b(di, dj) = its value at (i + di, j + dj, k). G_u += x_dot_g_b, G_v += y_dot_g_b
// (nonhydrostatic_tendency_kernel_functions.jl:95,157) on tendencies holding the advective part.
// ---------------------------------------------------------------------------------------------------------------------
template <class Q>
__device__ __forceinline__ double x_dot_g_b(const DGrid &g, double ghat_x, Q b) {
    return ghat_x * (g.tx == OCN_FLAT ? b(0, 0) : 0.5 * (b(-1, 0) + b(0, 0)));
}
template <class Q>
__device__ __forceinline__ double y_dot_g_b(const DGrid &g, double ghat_y, Q b) {
    return ghat_y * (g.ty == OCN_FLAT ? b(0, 0) : 0.5 * (b(0, -1) + b(0, 0)));
}
// buoyancy_perturbationᶜᶜᶜ with a compile-time kind (the run-time test of buoyancy_perturbation puts a branch around the S load)
template <int KIND>
__device__ __forceinline__ double buoyancy_perturbation_of(const double *bT, const double *S, double grav, double alpha, double beta, long q) {
    return KIND == 1 ? bT[q] : grav * (alpha * bT[q] - beta * S[q]);
}

template <int KIND>
__global__ void __launch_bounds__(256) buoyancy_acceleration_kernel(DGrid g, FView c, BuoyancyArgs B, double ghat_x, double ghat_y, FView Gu,
                                                                    FView Gv, Range6 ru, Range6 rv) {
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x;
    const int j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    const int k = 1 + blockIdx.z;
    if (i > g.Nx || j > g.Ny || k > g.Nz) return;
    auto b = [&](int di, int dj) { return buoyancy_perturbation_of<KIND>(B.bT, B.S, B.grav, B.alpha, B.beta, c.lin(i + di, j + dj, k)); };
    if (i >= ru.i0 && i <= ru.i1 && j >= ru.j0 && j <= ru.j1 && k >= ru.k0 && k <= ru.k1)
        Gu.at(i, j, k) = Gu.at(i, j, k) + x_dot_g_b(g, ghat_x, b);
    if (i >= rv.i0 && i <= rv.i1 && j >= rv.j0 && j <= rv.j1 && k >= rv.k0 && k <= rv.k1)
        Gv.at(i, j, k) = Gv.at(i, j, k) + y_dot_g_b(g, ghat_y, b);
}

// ---------------------------------------------------------------------------------------------------------------------
// stokes_drift = UniformStokesDrift(∂z_uˢ, ∂z_vˢ, ∂t_uˢ, ∂t_vˢ) (StokesDrifts.jl:39-178): a horizontally uniform surface-wave field, held as
// six per-level tables [k - 1]: ∂z_uˢ, ∂z_vˢ at centres (Nz) and at faces (Nz + 1), ∂t_uˢ, ∂t_vˢ at centres (Nz). A null table is a table
// of zeros -- the product is still formed, as the reference multiplies by its zerofunction. x_curl_Uˢ_cross_U = ℑxzᶠᵃᶜ(w) ∂z_uˢ(z_c),
// y_curl_Uˢ_cross_U = ℑyzᵃᶠᶜ(w) ∂z_vˢ(z_c), z_curl_Uˢ_cross_U = (-ℑxzᶜᵃᶠ(u)) ∂z_uˢ(z_f) - ℑyzᵃᶜᶠ(v) ∂z_vˢ(z_f) (:170-178) with ℑxz = ℑz(ℑx ·)
// (Operators/interpolation_operators.jl:8-15,50-56; the identity along a Flat direction). The velocities are read through accessors
// q(di, dj, dk) = value at (i + di, j + dj, k + dk), never called with an offset along a Flat direction: one body for the stand-alone kernel
// and the epilogue. k is the same for every lane of a wave, so the table values are scalar loads.
// ---------------------------------------------------------------------------------------------------------------------
struct StokesTables {
    const double *dzu_c, *dzu_f, *dzv_c, *dzv_f, *dtu_c, *dtv_c;
};
__device__ __forceinline__ double stokes_table(const double *t, int k) { return t ? t[k - 1] : 0.0; }
template <class QW>
__device__ __forceinline__ double x_curl_Us_cross_U(const DGrid &g, const StokesTables &sd, QW w, int k) {
    const bool flx = g.tx == OCN_FLAT, flz = g.tz == OCN_FLAT;
    auto X = [&](int dk) { return flx ? w(0, 0, dk) : 0.5 * (w(-1, 0, dk) + w(0, 0, dk)); };       // ℑxᶠᵃᵃ
    return (flz ? X(0) : 0.5 * (X(0) + X(1))) * stokes_table(sd.dzu_c, k);                       // ℑzᵃᵃᶜ (:170-171)
}
template <class QW>
__device__ __forceinline__ double y_curl_Us_cross_U(const DGrid &g, const StokesTables &sd, QW w, int k) {
    const bool fly = g.ty == OCN_FLAT, flz = g.tz == OCN_FLAT;
    auto Y = [&](int dk) { return fly ? w(0, 0, dk) : 0.5 * (w(0, -1, dk) + w(0, 0, dk)); };       // ℑyᵃᶠᵃ
    return (flz ? Y(0) : 0.5 * (Y(0) + Y(1))) * stokes_table(sd.dzv_c, k);                       // ℑzᵃᵃᶜ (:173-174)
}
template <class QU, class QV>
__device__ __forceinline__ double z_curl_Us_cross_U(const DGrid &g, const StokesTables &sd, QU u, QV v, int k) {
    const bool flx = g.tx == OCN_FLAT, fly = g.ty == OCN_FLAT, flz = g.tz == OCN_FLAT;
    auto X = [&](int dk) { return flx ? u(0, 0, dk) : 0.5 * (u(0, 0, dk) + u(1, 0, dk)); };        // ℑxᶜᵃᵃ
    auto Y = [&](int dk) { return fly ? v(0, 0, dk) : 0.5 * (v(0, 0, dk) + v(0, 1, dk)); };        // ℑyᵃᶜᵃ
    const double ua = flz ? X(0) : 0.5 * (X(-1) + X(0)), va = flz ? Y(0) : 0.5 * (Y(-1) + Y(0));   // ℑzᵃᵃᶠ
    return (-ua) * stokes_table(sd.dzu_f, k) - va * stokes_table(sd.dzv_f, k);                   // (:176-178)
}
// G = ((G_rest + curl) + ∂t_Uˢ) of each velocity (nonhydrostatic_tendency_kernel_functions.jl:100-101,162-163,226-227; ∂t_wˢ = zero(grid))
template <class QW>
__device__ __forceinline__ double stokes_Gu(const DGrid &g, const StokesTables &sd, QW w, int k, double G) {
    return (G + x_curl_Us_cross_U(g, sd, w, k)) + stokes_table(sd.dtu_c, k);
}
template <class QW>
__device__ __forceinline__ double stokes_Gv(const DGrid &g, const StokesTables &sd, QW w, int k, double G) {
    return (G + y_curl_Us_cross_U(g, sd, w, k)) + stokes_table(sd.dtv_c, k);
}
template <class QU, class QV>
__device__ __forceinline__ double stokes_Gw(const DGrid &g, const StokesTables &sd, QU u, QV v, int k, double G) {
    return (G + z_curl_Us_cross_U(g, sd, u, v, k)) + 0.0;
}

// the three terms on tendencies that hold everything up to the closure; each velocity over its own range, one thread per cell (i, j, k) of
// all three (w[k], w[k + 1] feed both G_u and G_v)
__global__ void __launch_bounds__(256) stokes_drift_kernel(DGrid g, StokesTables sd, FView u, FView v, FView w, FView Gu, FView Gv, FView Gw,
                                                           Range6 ru, Range6 rv, Range6 rw) {
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x;
    const int j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    const int k = 1 + blockIdx.z;
    if (i > g.Nx || j > g.Ny || k > g.Nz) return;
    auto qu = [&](int di, int dj, int dk) { return u.at(i + di, j + dj, k + dk); };
    auto qv = [&](int di, int dj, int dk) { return v.at(i + di, j + dj, k + dk); };
    auto qw = [&](int di, int dj, int dk) { return w.at(i + di, j + dj, k + dk); };
    if (i >= ru.i0 && i <= ru.i1 && j >= ru.j0 && j <= ru.j1 && k >= ru.k0 && k <= ru.k1)
        Gu.at(i, j, k) = stokes_Gu(g, sd, qw, k, Gu.at(i, j, k));
    if (i >= rv.i0 && i <= rv.i1 && j >= rv.j0 && j <= rv.j1 && k >= rv.k0 && k <= rv.k1)
        Gv.at(i, j, k) = stokes_Gv(g, sd, qw, k, Gv.at(i, j, k));
    if (i >= rw.i0 && i <= rw.i1 && j >= rw.j0 && j <= rw.j1 && k >= rw.k0 && k <= rw.k1)
        Gw.at(i, j, k) = stokes_Gw(g, sd, qu, qv, k, Gw.at(i, j, k));
}

// ---------------------------------------------------------------------------------------------------------------------
// One pass for everything that follows the advective part of the tendencies (nonhydrostatic_tendency_kernel_functions.jl:91-100,
// 153-162,216-229,286-297): G = (((A - f×U) - ∇pHY′) - ∂ⱼτᵢⱼ) + 0 for every prognostic field, and -- optionally -- the RK3 substep
// of the NEXT stage into the second set of prognostic arrays (the viscous stencils of neighbouring cells still read U). The
// terms are the device functions of the stand-alone kernels above, evaluated in the reference's order => identical bits.
// ---------------------------------------------------------------------------------------------------------------------
#define OCN_EPILOGUE_MAX_LIN 12
struct EpilogueArgs {
    int n, ntr;
    FView u, v, w, c[OCN_MAX_FIELDS], pHY;      // .p of the views = the live fields
    double *Gn[OCN_MAX_FIELDS];
    const double *Gm[OCN_MAX_FIELDS];
    double *Un[OCN_MAX_FIELDS];
    Range6 r[OCN_MAX_FIELDS];
    bool has_coriolis, has_buoyancy, substep, has_zeta;
    bool store_G;                               // false: the completed tendency feeds the substep riding along and nothing else (FusedSubstep::store_G)
    int store_sides;                            // ... except on these sides (bit = side): epilogue_flux_shell_kernel re-does their cells from the stored value
    double fcor, nu, kappa[OCN_MAX_FIELDS], dt, gamma, zeta;
    bool amd;                                   // eddy coefficients from arrays (AnisotropicMinimumDissipation, Smagorinsky)
    FView nu_e, kappa_e[OCN_MAX_FIELDS];
    // valued Flux boundary conditions (compute_flux_bcs.jl:57-163), applied after the interior terms: [field][side]
    bool any_flux;
    bool has_flux[OCN_MAX_FIELDS][6];
    double flux[OCN_MAX_FIELDS][6];
    const double *flux_arr[OCN_MAX_FIELDS][6];  // array-valued Flux conditions (null: the number above)
    int loc[OCN_MAX_FIELDS][3];
    // linear field-dependent Flux conditions flux = a + b φ (linear_flux_bc_kernel), applied after the valued ones in (field, side)
    // order like the stand-alone launches
    int nlin;
    struct Lin { int f, side, dep; double a, b; } lin[OCN_EPILOGUE_MAX_LIN];
    // ConstantCartesianCoriolis and BuoyancyForce(gravity_unit_vector) (the EXT instantiations of tendency_epilogue_kernel): the rotation
    // vector, ĝ_x, ĝ_y and what buoyancy_perturbation needs. At the end: every member above keeps its place in the kernel arguments
    double cfx, cfy, cfz, ghat_x, ghat_y;
    const double *bT, *bS;
    double grav, alpha, beta;
};

// the valued and the linear field-dependent Flux conditions of field f at (i, j, k) (parent index q), applied to a tendency G that holds
// the interior terms
__device__ __forceinline__ double epilogue_flux_conditions(const DGrid &g, const EpilogueArgs &a, int f, int i, int j, int k, long q, double G) {
    if (a.any_flux) {
        // compute_x/y/z_bcs!: G[1] += flux A / V, G[N] -= flux A / V (x, then y, then z as the reference launches them)
        const int N[3] = {g.Nx, g.Ny, g.Nz}, idx[3] = {i, j, k};
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            // tangential point of the condition: (j, k) on west / east, (i, k) on south / north, (i, j) on bottom / top
            const long ab = d == 0 ? (long)(j - 1) + (long)g.Ny * (k - 1) : (d == 1 ? (long)(i - 1) + (long)g.Nx * (k - 1) : (long)(i - 1) + (long)g.Nx * (j - 1));
#pragma unroll
            for (int side = 0; side < 2; ++side) {
                const int sd = 2 * d + side;
                if (!a.has_flux[f][sd] || idx[d] != (side ? N[d] : 1)) continue;
                const double *fa = a.flux_arr[f][sd];
                G = add_flux_condition(g, d, a.loc[f][2], k, side, fa ? fa[ab] : a.flux[f][sd], G);
            }
        }
    }
    for (int n = 0; n < a.nlin; ++n) {
        if (a.lin[n].f != f) continue;
        const int sd = a.lin[n].side, d = sd >> 1, dep = a.lin[n].dep;
        const int idxd = d == 0 ? i : (d == 1 ? j : k), Nd = d == 0 ? g.Nx : (d == 1 ? g.Ny : g.Nz);
        if (idxd != ((sd & 1) ? Nd : 1)) continue;
        const double *dp = dep == 0 ? a.u.p : (dep == 1 ? a.v.p : (dep == 2 ? a.w.p : a.c[dep - 3].p));
        // the dependency sits at the location of the field: same parent index
        G = add_flux_condition(g, d, a.loc[f][2], k, sd & 1, linear_flux(a.lin[n].a, a.lin[n].b, dp[q]), G);
    }
    return G;
}

// COR / BUOY / CLO (0 none, 1 constant ν, κ, 2 eddy-coefficient arrays, 3 the same with the tracers' interpolated coefficient divided by
// the Prandtl number that a.kappa[t] then holds -- Smagorinsky with Pr ≠ 1, 4 constant ν, κ with the explicit part of a vertically implicit
// time discretisation) are compile-time: the terms of one cell then form ONE basic
// block whose ~40 loads the compiler issues together -- with run-time flags every term was its own block behind a branch and its
// loads waited one after the other (0.94 -> see DESIGN.md for the measured time at 256 x 256 x 128).
// EXT (bits; 0: the kernel as it was): 1 -- the Coriolis term is ConstantCartesianCoriolis (with COR; then w has one too); 2 -- the buoyancy
// has a gravity_unit_vector (with BUOY): x_dot_g_b / y_dot_g_b come first after the advective part, before Coriolis
// (nonhydrostatic_tendency_kernel_functions.jl:95-97,157-159,222-223); 4 -- its buoyancy perturbation is g (α T - β S) instead of the tracer.
// STOKES: the terms of a UniformStokesDrift follow the closure term of each velocity. Their tables ride behind the arguments in a struct
// of the STOKES instantiations only, so EpilogueArgs, the instantiations without the terms and every other kernel that takes it keep their
// code (shared through a __device__ function instead, the scalar code of all 60 existing instantiations changed).
struct EpilogueStokesArgs : EpilogueArgs { StokesTables sd; };
template <bool STOKES> struct EpilogueArgsOf { typedef EpilogueArgs type; };
template <> struct EpilogueArgsOf<true> { typedef EpilogueStokesArgs type; };
template <bool COR, bool BUOY, int CLO, int EXT = 0, bool STOKES = false>
__global__ void __launch_bounds__(256) tendency_epilogue_kernel(DGrid g, typename EpilogueArgsOf<STOKES>::type a) {
    // 0.66 ms at 256 x 256 x 128 with the configs[4] physics: ~200 loads per cell, bound on the address / L1 path (VALU busy < 50 %, 3.5 TB/s). Grids without
    // a Flat direction run tendency_epilogue_march_kernel (ocn_epilogue_march.h, 0.48 ms) instead; this kernel stays for the others and as its reference.
    const int f = blockIdx.z % a.n;
    const Range6 r = a.r[f];
    const int i = r.i0 + blockIdx.x * blockDim.x + threadIdx.x;
    const int j = r.j0 + blockIdx.y * blockDim.y + threadIdx.y;
    const int k = r.k0 + blockIdx.z / a.n;
    if (i > r.i1 || j > r.j1 || k > r.k1) return;
    const FView &fv = f == 0 ? a.u : (f == 1 ? a.v : (f == 2 ? a.w : a.c[f - 3]));
    const long q = fv.lin(i, j, k);
    double G = a.Gn[f][q];
    constexpr bool VAR = CLO == 2 || CLO == 3, PRD = CLO == 3, VI = CLO == 4;
    constexpr bool CART = (EXT & 1) != 0, TILT = (EXT & 2) != 0;
    constexpr int BKIND = (EXT & 4) ? 2 : 1;
    auto qu = [&](int di, int dj, int dk) { return a.u.at(i + di, j + dj, k + dk); };
    auto qv = [&](int di, int dj, int dk) { return a.v.at(i + di, j + dj, k + dk); };
    auto qw = [&](int di, int dj, int dk) { return a.w.at(i + di, j + dj, k + dk); };
    auto qb = [&](int di, int dj) { return buoyancy_perturbation_of<BKIND>(a.bT, a.bS, a.grav, a.alpha, a.beta, a.pHY.lin(i + di, j + dj, k)); };
    if (f == 0) {
        if (TILT) G = G + x_dot_g_b(g, a.ghat_x, qb);
        if (COR && CART) G = G - x_f_cross_U_cartesian(g, a.cfy, a.cfz, qv, qw);
        if (COR && !CART) G = G - x_f_cross_U(g, a.fcor, a.v, i, j, k);
        if (BUOY) G = G - hydrostatic_gradient_x(g, a.pHY, i, j, k);
        if (CLO && (VAR || a.nu != 0.0)) G = (G - closure_divergence<F_U, false, VI>(g, a.u, a.v, a.w, a.u, a.nu, i, j, k, VAR, a.nu_e)) + 0.0;
        if constexpr (STOKES) G = stokes_Gu(g, a.sd, qw, k, G);
    } else if (f == 1) {
        if (TILT) G = G + y_dot_g_b(g, a.ghat_y, qb);
        if (COR && CART) G = G - y_f_cross_U_cartesian(g, a.cfx, a.cfz, qu, qw);
        if (COR && !CART) G = G - y_f_cross_U(g, a.fcor, a.u, i, j, k);
        if (BUOY) G = G - hydrostatic_gradient_y(g, a.pHY, i, j, k);
        if (CLO && (VAR || a.nu != 0.0)) G = (G - closure_divergence<F_V, false, VI>(g, a.u, a.v, a.w, a.u, a.nu, i, j, k, VAR, a.nu_e)) + 0.0;
        if constexpr (STOKES) G = stokes_Gv(g, a.sd, qw, k, G);
    } else if (f == 2) {
        if (COR && CART) G = G - z_f_cross_U_cartesian(g, a.cfx, a.cfy, qu, qv);
        if (CLO && (VAR || a.nu != 0.0)) G = (G - closure_divergence<F_W, false, VI>(g, a.u, a.v, a.w, a.u, a.nu, i, j, k, VAR, a.nu_e)) + 0.0;
        if constexpr (STOKES) G = stokes_Gw(g, a.sd, qu, qv, k, G);
    } else {
        const double kap = a.kappa[f - 3];
        if (CLO && (VAR || kap != 0.0))
            G = (G - closure_divergence<F_C, PRD, VI>(g, a.u, a.v, a.w, a.c[f - 3], kap, i, j, k, VAR, a.kappa_e[f - 3])) + 0.0;
    }
    G = epilogue_flux_conditions(g, a, f, i, j, k, q, G);
    if (a.store_G) a.Gn[f][q] = G;
    if (a.substep) {
        double Uv = fv.p[q];
        if (a.has_zeta) Uv += a.dt * (a.gamma * G + a.zeta * a.Gm[f][q]);
        else            Uv += a.dt * a.gamma * G;
        a.Un[f][q] = Uv;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// RK3 substep / tendency caching (src/TimeSteppers/runge_kutta_3.jl:212-226, store_tendencies.jl:6-9)
// ---------------------------------------------------------------------------------------------------------------------
struct SubstepArgs {
    double *U[OCN_MAX_FIELDS];
    const double *Gn[OCN_MAX_FIELDS];
    const double *Gm[OCN_MAX_FIELDS];
    FView view[OCN_MAX_FIELDS];     // .p unused
    Range6 r[OCN_MAX_FIELDS];
    int n;
};

__global__ void __launch_bounds__(256) rk3_substep_kernel(SubstepArgs a, double dt, double gamma, double zeta, bool has_zeta) {
    const int f = blockIdx.z % a.n;
    const Range6 r = a.r[f];
    const int i = r.i0 + blockIdx.x * blockDim.x + threadIdx.x;
    const int j = r.j0 + blockIdx.y * blockDim.y + threadIdx.y;
    const int k = r.k0 + blockIdx.z / a.n;
    if (i > r.i1 || j > r.j1 || k > r.k1) return;
    const long q = a.view[f].lin(i, j, k);
    double Uv = a.U[f][q];
    if (has_zeta) Uv += dt * (gamma * a.Gn[f][q] + zeta * a.Gm[f][q]);
    else          Uv += dt * gamma * a.Gn[f][q];
    a.U[f][q] = Uv;
}

// ab2_step_field! (TimeSteppers/quasi_adams_bashforth_2.jl:160-173): Gu = (1.5 + χ) Gⁿ - (0.5 + χ) G⁻ * not_euler; u += Δt Gu
__global__ void __launch_bounds__(256) ab2_step_kernel(SubstepArgs a, double dt, double chi) {
    const int f = blockIdx.z % a.n;
    const Range6 r = a.r[f];
    const int i = r.i0 + blockIdx.x * blockDim.x + threadIdx.x;
    const int j = r.j0 + blockIdx.y * blockDim.y + threadIdx.y;
    const int k = r.k0 + blockIdx.z / a.n;
    if (i > r.i1 || j > r.j1 || k > r.k1) return;
    const long q = a.view[f].lin(i, j, k);
    const bool not_euler = chi != -0.5;            // `* false` is a strong zero: leftover NaNs in G⁻ cannot leak into a Euler step
    const double prev = not_euler ? (0.5 + chi) * a.Gm[f][q] * 1.0 : 0.0;
    const double Gu = (1.5 + chi) * a.Gn[f][q] - prev;
    a.U[f][q] += dt * Gu;
}

__global__ void __launch_bounds__(256) cache_tendencies_kernel(SubstepArgs a) {
    const int f = blockIdx.z % a.n;
    const Range6 r = a.r[f];
    const int i = r.i0 + blockIdx.x * blockDim.x + threadIdx.x;
    const int j = r.j0 + blockIdx.y * blockDim.y + threadIdx.y;
    const int k = r.k0 + blockIdx.z / a.n;
    if (i > r.i1 || j > r.j1 || k > r.k1) return;
    const long q = a.view[f].lin(i, j, k);
    a.U[f][q] = a.Gn[f][q];
}

// ---------------------------------------------------------------------------------------------------------------------
// Poisson solvers (src/Solvers)
// ---------------------------------------------------------------------------------------------------------------------
// `@. ϕc = -b / (λx + λy + λz - m)` with m = 0 and `ϕc[1,1,1] = 0` (fft_based_poisson_solver.jl:110,115)
// Nxs = stored row length (Nx for complex-to-complex, Nx/2+1 for the Hermitian half spectrum of the real transform);
// `scale` folds the inverse-FFT normalisation 1/prod(N) into the same pass when apply_scale is set.
__global__ void __launch_bounds__(256) spectral_divide_kernel(double2 *b, const double *lx, const double *ly, const double *lz,
                                                              int Nxs, int Ny, int Nz, double scale, bool apply_scale) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = blockIdx.y * blockDim.y + threadIdx.y;
    const int k = blockIdx.z;
    if (i >= Nxs || j >= Ny || k >= Nz) return;
    const long q = (long)i + (long)Nxs * (j + (long)Ny * k);
    double lam = (lx[i] + ly[j]) + lz[k] - 0.0;
    double2 val = b[q];
    val.x = -val.x / lam;
    val.y = -val.y / lam;
    if (apply_scale) { val.x *= scale; val.y *= scale; }
    if (q == 0) { val.x = 0.0; val.y = 0.0; }
    b[q] = val;
}

// copy_real_component! (fft_based_poisson_solver.jl:129-137) fused with the ifft normalisation (AbstractFFTs ScaledPlan:
// multiply by 1/prod(N)) and, for the Fourier-tridiagonal solver, the mean removal
// `ϕ .= ϕ .- mean(ϕ)` (fourier_tridiagonal_poisson_solver.jl:233): real(ϕ*scale - mean).
__global__ void __launch_bounds__(256) copy_real_kernel(DGrid g, FView phi, const double2 *src, double scale, bool apply_scale,
                                                        const double2 *mean) {
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x;
    const int j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    const int k = 1 + blockIdx.z;
    if (i > g.Nx || j > g.Ny || k > g.Nz) return;
    double val = src[(long)(i - 1) + (long)g.Nx * ((j - 1) + (long)g.Ny * (k - 1))].x;
    if (apply_scale) val *= scale;
    if (mean) val -= mean->x;
    phi.at(i, j, k) = val;
}

// solve_batched_tridiagonal_system_kernel! z direction (batched_tridiagonal_solver.jl:213-245): one thread per (i, j)
// column, coalesced across i. Complex f / phi, real a, b (3-D), c, scratch t (3-D real).
// Nxs columns per row are solved; f / phi have row length Nxs, the real coefficient arrays b / t row length ldb
// (ldb = Nx > Nxs = Nx/2+1 when only the Hermitian half spectrum is solved). fscale multiplies the right-hand side
// (1 for the reference semantics; the folded inverse-FFT normalisation on the real-transform path).
__global__ void __launch_bounds__(64) tridiagonal_z_kernel(int Nxs, int ldb, int Ny, int Nz, const double *__restrict__ a,
                                                           const double *__restrict__ b, const double *__restrict__ c,
                                                           const double2 *__restrict__ f, double *__restrict__ t,
                                                           double2 *__restrict__ phi, double fscale, bool apply_scale, int ldf = 0) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = blockIdx.y;
    if (i >= Nxs || j >= Ny) return;
    const int ldx = ldf > 0 ? ldf : Nxs;              // row pitch of f / phi
    const long st = (long)ldx * Ny, stb = (long)ldb * Ny;
    long q = (long)i + (long)ldx * j, qb = (long)i + (long)ldb * j;
    double beta = b[qb];
    double2 f1 = f[q];
    if (apply_scale) { f1.x *= fscale; f1.y *= fscale; }
    double2 prev = make_double2(f1.x / beta, f1.y / beta);
    phi[q] = prev;
    // The recurrences are serial in k, but every load is independent of them: with < 1 wave per SIMD (Nxs * Ny columns only)
    // the kernel is pure memory latency unless the loads of several levels are in flight together => blocks of TB levels are
    // fetched into registers first, then swept.
    constexpr int TB = 8;
    for (int k0 = 1; k0 < Nz; k0 += TB) {
        double2 fb[TB], ob[TB];
        double bb[TB], cb[TB], ab[TB];
#pragma unroll
        for (int n = 0; n < TB; ++n) {
            const int k = k0 + n;
            if (k < Nz) {
                fb[n] = f[q + (long)(n + 1) * st]; ob[n] = phi[q + (long)(n + 1) * st]; bb[n] = b[qb + (long)(n + 1) * stb];
                cb[n] = c[k - 1]; ab[n] = a[k - 1];
            }
        }
#pragma unroll
        for (int n = 0; n < TB; ++n) {
            const int k = k0 + n;
            if (k < Nz) {
                q += st; qb += stb;
                const double ck1 = cb[n], ak1 = ab[n], bk = bb[n];
                const double tk = ck1 / beta;
                t[qb] = tk;
                beta = bk - ak1 * tk;
                double2 fk = fb[n];
                if (apply_scale) { fk.x *= fscale; fk.y *= fscale; }
                const bool dd = fabs(beta) > 10.0 * 2.220446049250313e-16;
                const double2 star = make_double2((fk.x - ak1 * prev.x) / beta, (fk.y - ak1 * prev.y) / beta);
                prev = dd ? star : ob[n];
                phi[q] = prev;
            }
        }
    }
    for (int k0 = Nz - 2; k0 >= 0; k0 -= TB) {
        double tb[TB];
        double2 pb[TB];
#pragma unroll
        for (int n = 0; n < TB; ++n) {
            const int k = k0 - n;
            if (k >= 0) { tb[n] = t[qb - (long)n * stb]; pb[n] = phi[q - (long)(n + 1) * st]; }     // t[k+1], phi[k]
        }
#pragma unroll
        for (int n = 0; n < TB; ++n) {
            const int k = k0 - n;
            if (k >= 0) {
                q -= st; qb -= stb;
                double2 cur = pb[n];
                cur.x -= tb[n] * prev.x;
                cur.y -= tb[n] * prev.y;
                phi[q] = cur;
                prev = cur;
            }
        }
    }
}

// `ϕ .= ϕ .- mean(ϕ)` (fourier_tridiagonal_poisson_solver.jl:233) applied in spectral space: the volume mean lives in
// the (kx, ky) = (0, 0) column, mean(ϕ) * Nx*Ny = mean_k ϕ̂(0,0,k). One workgroup.
__global__ void __launch_bounds__(256) remove_mean_mode_kernel(double2 *phi, long plane_stride, int Nz) {
    __shared__ double sx[256], sy[256];
    double ax = 0, ay = 0;
    for (int k = threadIdx.x; k < Nz; k += 256) { ax += phi[k * plane_stride].x; ay += phi[k * plane_stride].y; }
    sx[threadIdx.x] = ax; sy[threadIdx.x] = ay;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) { sx[threadIdx.x] += sx[threadIdx.x + s]; sy[threadIdx.x] += sy[threadIdx.x + s]; }
        __syncthreads();
    }
    const double mx = sx[0] / (double)Nz, my = sy[0] / (double)Nz;
    for (int k = threadIdx.x; k < Nz; k += 256) { phi[k * plane_stride].x -= mx; phi[k * plane_stride].y -= my; }
}

// ---------------------------------------------------------------------------------------------------------------------
// Irregular x partitions (remainder columns on the last rank, distributed_grids.jl:44-58): the gathered pressure solve. Every rank
// contributes its source term with rows padded to the widest slab (nmax columns); assemble the global dense right-hand side from
// the R gathered pieces, and -- after the single-GPU solver ran on it -- take the own slab back out of the global solution.
// first[q] = global index (0-based) of rank q's first column, first[R] = Nx_global.
// ---------------------------------------------------------------------------------------------------------------------
// With a pencil (Rx x Ry) partition the pieces are (nxmax, nymax, Nz) blocks, rank = ix * Ry + iy (index2rank, distributed_architectures.jl:354).
#define OCN_MAX_RANKS 64
struct SlabTable { int first[OCN_MAX_RANKS + 1]; int R; int firsty[OCN_MAX_RANKS + 1]; int Ry; };
template <bool COMPLEX>
__global__ void __launch_bounds__(256) gather_assemble_kernel(const double *all, void *dst, SlabTable t, int nmax, int nymax, int Nxg, int Nyg, int Nz) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = blockIdx.y * blockDim.y + threadIdx.y;
    const int k = blockIdx.z;
    if (i >= Nxg || j >= Nyg || k >= Nz) return;
    int q = 0, qy = 0;
    while (q + 1 < t.R && i >= t.first[q + 1]) ++q;
    while (qy + 1 < t.Ry && j >= t.firsty[qy + 1]) ++qy;
    const size_t r = (size_t)q * t.Ry + qy;
    const double v = all[(size_t)(i - t.first[q]) + (size_t)nmax * ((j - t.firsty[qy]) + (size_t)nymax * (k + (size_t)Nz * r))];
    const size_t d = (size_t)i + (size_t)Nxg * (j + (size_t)Nyg * k);
    if (COMPLEX) ((double2 *)dst)[d] = make_double2(v, 0.0);
    else ((double *)dst)[d] = v;
}
// local haloed phi(i, j, k) = global haloed gphi(off + i, offy + j, k) over the local interior
__global__ void __launch_bounds__(256) slab_extract_kernel(DGrid g, FView phi, FView gphi, int off, int offy) {
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x;
    const int j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    const int k = 1 + blockIdx.z;
    if (i > g.Nx || j > g.Ny || k > g.Nz) return;
    phi.at(i, j, k) = gphi.at(off + i, offy + j, k);
}

// ---------------------------------------------------------------------------------------------------------------------
// Per-dimension transforms for grids with Bounded (cosine-transform) directions -- DiscreteTransform on the GPU
// (Solvers/discrete_transforms.jl:108-175, index_permutations.jl:18-72, plan_transforms.jl:39-136).
// Each direction d is transformed on its own: GATHER the lines of A (Nx, Ny, Nz) along d into a line-contiguous buffer B
// (B[m + N*line]), run ONE unit-stride batched complex FFT, SCATTER back. The cosine transforms ride on the same FFT
// (Makhoul 1980): forward  v = even-odd permutation of x, V = FFT(v), Y[k] = 2 Re(e^{-iπk/2N} V[k])   (= FFTW REDFT10);
// backward V[k] = e^{iπk/2N} (Y[k] - i Y[N-k]) / 2, v = N * IFFT(V), x = unpermuted v  -- i.e. N x like an unnormalised
// inverse FFT, so every direction contributes the same 1/N to the normalisation. Bounded directions are transformed FIRST
// on the way in and LAST on the way out (plan_transforms.jl:44-65) so that their input is real.
// mode 0: Periodic (plain copy); 1: Bounded forward; 2: Bounded backward.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int line_perm(int n, int N) { return (n & 1) ? N - 1 - (n >> 1) : (n >> 1); }

__global__ void __launch_bounds__(256) line_gather_kernel(const double2 *A, double2 *B, int Nx, int Ny, int Nz, int d, int mode) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = blockIdx.y * blockDim.y + threadIdx.y;
    const int k = blockIdx.z;
    if (i >= Nx || j >= Ny || k >= Nz) return;
    const long sx = 1, sy = Nx, sz = (long)Nx * Ny;
    const long q = i * sx + j * sy + k * sz;
    const int n = d == 0 ? i : (d == 1 ? j : k);
    const int N = d == 0 ? Nx : (d == 1 ? Ny : Nz);
    const long sd = d == 0 ? sx : (d == 1 ? sy : sz);
    const long line = d == 0 ? (j + (long)Ny * k) : (d == 1 ? (i + (long)Nx * k) : (i + (long)Nx * j));
    double2 val = A[q];
    int m = n;
    if (mode == 1) {
        m = line_perm(n, N);
        val.y = 0.0;
    } else if (mode == 2) {
        const double yk = val.x;
        const double ynk = n == 0 ? 0.0 : A[q + (long)(N - 2 * n) * sd].x;     // Y[N - n], Y[N] := 0
        double sn, cs;
        sincospi((double)n / (2.0 * (double)N), &sn, &cs);
        // e^{iπn/2N} (yk - i ynk) / 2
        val = make_double2(0.5 * (cs * yk + sn * ynk), 0.5 * (sn * yk - cs * ynk));
    }
    B[m + (long)N * line] = val;
}

__global__ void __launch_bounds__(256) line_scatter_kernel(const double2 *B, double2 *A, int Nx, int Ny, int Nz, int d, int mode) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = blockIdx.y * blockDim.y + threadIdx.y;
    const int k = blockIdx.z;
    if (i >= Nx || j >= Ny || k >= Nz) return;
    const long q = i + (long)Nx * (j + (long)Ny * k);
    const int n = d == 0 ? i : (d == 1 ? j : k);
    const int N = d == 0 ? Nx : (d == 1 ? Ny : Nz);
    const long line = d == 0 ? (j + (long)Ny * k) : (d == 1 ? (i + (long)Nx * k) : (i + (long)Nx * j));
    if (mode == 0) {
        A[q] = B[n + (long)N * line];
    } else if (mode == 1) {
        const double2 V = B[n + (long)N * line];
        double sn, cs;
        sincospi((double)n / (2.0 * (double)N), &sn, &cs);
        A[q] = make_double2(2.0 * (cs * V.x + sn * V.y), 0.0);                   // 2 Re(e^{-iπn/2N} V)
    } else {
        A[q] = make_double2(B[line_perm(n, N) + (long)N * line].x, 0.0);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Substructured x solve of the distributed FFT Poisson solver (z Periodic): after the local (y, z) transform every (ky, kz) mode
// is an independent PERIODIC CONSTANT-COEFFICIENT TRIDIAGONAL system along the partitioned x direction,
//     a (p[i-1] - 2 p[i] + p[i+1]) - (λy + λz) p[i] = r[i],   a = 1/Δx².
// Instead of transposing the whole spectrum twice (2 all-to-alls of ~140 MB per rank -- one xGMI link per peer) each rank solves
// its slab with Dirichlet ends (Thomas, real coefficients precomputed once), the ranks exchange TWO numbers per mode (first and
// last value: an all-gather of ~1 MB), the 2R interface unknowns per mode follow from a system that is block-circulant in the
// rank index (constant coefficients => diagonalised by an R-point DFT: 2x2 solves), and the slab solution is corrected with
// p = y - a gL s - a gR s[reversed], s = T⁻¹ e₀. The null mode (ky = kz = 0) is pinned and shifted to zero mean like the
// reference's ϕ̂[1,1,1] = 0. Same solution as the transposed FFT solve to round-off (tested at 1e-12).
// Spectral layout here: Y[m + M*i], m = ky + Nyh*kz fastest (coalesced sweeps along x), i = local x index.
// ---------------------------------------------------------------------------------------------------------------------
// setup, one thread per mode: rden[i] = 1 / (b - a cp[i-1]), cp[i] = a rden[i], s = T⁻¹ e₀ (T = tridiag(a, b, a), b = -2a - λ)
__global__ void __launch_bounds__(256) sub_setup_kernel(int M, int Nyh, int N, double a, const double *ly, const double *lz, double *rden,
                                                        double *cp, double *svec, double *ssum0) {
    const long m = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const int jy = m % Nyh, k = m / Nyh;
    const double b = -2.0 * a - (ly[jy] + lz[k]);
    double c = 0.0;
    for (int i = 0; i < N; ++i) {
        const double rd = 1.0 / (b - a * c);
        c = a * rd;
        rden[m + (long)M * i] = rd;
        cp[m + (long)M * i] = c;
    }
    double y = rden[m];                       // forward sweep of e₀: y[0] = 1/den[0], y[i] = -a y[i-1] / den[i]
    svec[m] = y;
    for (int i = 1; i < N; ++i) { y = (-a * y) * rden[m + (long)M * i]; svec[m + (long)M * i] = y; }
    for (int i = N - 2; i >= 0; --i) svec[m + (long)M * i] -= cp[m + (long)M * i] * svec[m + (long)M * (i + 1)];
    if (m == 0) {                             // Σ_i s[i] of the null mode (its global mean needs it at every solve)
        double t = 0.0;
        for (int i = 0; i < N; ++i) t += svec[(long)M * i];
        *ssum0 = t;
    }
}

// separate the paired columns (see dist_pack_forward_kernel) and transpose (ih, k, j) -> (m, i) through an LDS tile
__global__ void __launch_bounds__(256) sub_separate_kernel(const double2 *Z, double2 *Y, int Nxl, int Nxh, int Ny, int Nyh, int Nz) {
    __shared__ double2 tA[16][17], tB[16][17];
    const int k = blockIdx.z, tx = threadIdx.x, ty = threadIdx.y;
    const long M = (long)Nyh * Nz;
    {
        const int ih = blockIdx.x * 16 + tx, j = blockIdx.y * 16 + ty;
        if (ih < Nxh && j < Nyh) {
            const int jm = j == 0 ? 0 : Ny - j, km = k == 0 ? 0 : Nz - k;
            const double2 z1 = Z[ih + (long)Nxh * (k + (long)Nz * j)], z2 = Z[ih + (long)Nxh * (km + (long)Nz * jm)];
            tA[ty][tx] = make_double2(0.5 * (z1.x + z2.x), 0.5 * (z1.y - z2.y));
            tB[ty][tx] = make_double2(0.5 * (z1.y + z2.y), 0.5 * (z2.x - z1.x));
        }
    }
    __syncthreads();
    {
        const int j = blockIdx.y * 16 + tx, ih = blockIdx.x * 16 + ty;
        if (ih < Nxh && j < Nyh) {
            const long m = j + (long)Nyh * k;
            Y[m + M * (2 * ih)] = tA[tx][ty];
            if (2 * ih + 1 < Nxl) Y[m + M * (2 * ih + 1)] = tB[tx][ty];
        }
    }
}

// Thomas sweeps along x for every mode (in place), then the payload: first / last value per mode and, for mode 0, the sum
// ZF: the spectrum is stored z-fastest, Y[kz + Nzp*(i + N*ky)] (row pitch Nzp >= Nzh) with m = kz + Nzh*ky (what R2C along z + a strided y transform leave
// behind); otherwise mode-fastest, Y[m + M*i]. The factor arrays are mode-fastest in both cases.
template <bool ZF>
__global__ void __launch_bounds__(64) sub_thomas_kernel(long M, int N, double a, const double *__restrict__ rden, const double *__restrict__ cp,
                                                        double2 *__restrict__ Yin, double2 *__restrict__ payload, int Nzh, int Nzp) {
    const long m = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    // element (m, i) of the spectrum: base + stride * i (ZF: rows of Nzh modes stored with pitch Nzp >= Nzh, whole 128-B lines)
    const long ybase = ZF ? (m % Nzh) + (long)Nzp * N * (m / Nzh) : m;
    const long ystride = ZF ? (long)Nzp : M;
    double2 *__restrict__ Y = Yin + ybase - m;          // so that Y[m + ystride * i] below is the element
    constexpr int TB = 8;
    double2 prev = make_double2(0.0, 0.0);
    for (int i0 = 0; i0 < N; i0 += TB) {
        double2 r[TB];
        double d[TB];
#pragma unroll
        for (int n = 0; n < TB; ++n)
            if (i0 + n < N) { r[n] = Y[m + ystride * (i0 + n)]; d[n] = rden[m + M * (i0 + n)]; }
#pragma unroll
        for (int n = 0; n < TB; ++n)
            if (i0 + n < N) {
                prev = make_double2((r[n].x - a * prev.x) * d[n], (r[n].y - a * prev.y) * d[n]);
                Y[m + ystride * (i0 + n)] = prev;
            }
    }
    double2 sum = prev;                           // prev = y[N-1] is final already
    const double2 last = prev;
    for (int i0 = N - 2; i0 >= 0; i0 -= TB) {
        double2 y[TB];
        double c[TB];
#pragma unroll
        for (int n = 0; n < TB; ++n)
            if (i0 - n >= 0) { y[n] = Y[m + ystride * (i0 - n)]; c[n] = cp[m + M * (i0 - n)]; }
#pragma unroll
        for (int n = 0; n < TB; ++n)
            if (i0 - n >= 0) {
                prev = make_double2(y[n].x - c[n] * prev.x, y[n].y - c[n] * prev.y);
                Y[m + ystride * (i0 - n)] = prev;
                sum.x += prev.x; sum.y += prev.y;
            }
    }
    payload[m] = prev;                            // y[0]
    payload[M + m] = last;                        // y[N-1]
    if (m == 0) payload[2 * M] = sum;
}

// interface unknowns from the gathered payloads (R ranks x (2M + 1)): per mode an R-point DFT over the rank index, 2x2 solves, and
// the two values this rank needs: gL = l[rank-1], gR = f[rank+1]. out[m] = gL, out[M+m] = gR, out[2M] = mean of mode 0
__global__ void __launch_bounds__(256) sub_interface_kernel(long M, int Nyh, int N, int R, int rank, double a, const double *ly,
                                                            const double *lz, const double *s_first, const double *s_last, const double *ssum0,
                                                            const double2 *gathered, double2 *out) {
    const long m = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const long stride = 2 * M + 1;
    const double alpha = a * s_first[m], beta = a * s_last[m];          // s = T⁻¹e₀: its first and its last entry
    const bool null_mode = m == 0 && (ly[0] + lz[0]) == 0.0;
    double2 gl = make_double2(0.0, 0.0), gr = gl;
    double2 mean = gl;
    const int rl = (rank + R - 1) % R, rr = (rank + 1) % R;
    for (int q = 0; q < R; ++q) {
        double2 yF = make_double2(0.0, 0.0), yL = yF;           // DFT over the rank index: Σ_r y_r e^{-2πi q r / R}
        for (int r = 0; r < R; ++r) {
            double sn, cs;
            sincospi(-2.0 * (double)((q * r) % R) / (double)R, &sn, &cs);
            const double2 f = gathered[r * stride + m], l = gathered[r * stride + M + m];
            yF.x += f.x * cs - f.y * sn; yF.y += f.x * sn + f.y * cs;
            yL.x += l.x * cs - l.y * sn; yL.y += l.x * sn + l.y * cs;
        }
        double so, co;
        sincospi(2.0 * (double)q / (double)R, &so, &co);        // ω = e^{2πi q / R}
        // [1 + β ω,  α ω⁻¹; α ω,  1 + β ω⁻¹] [f̂; l̂] = [ŷF; ŷL]
        const double2 A11 = make_double2(1.0 + beta * co, beta * so), A22 = make_double2(1.0 + beta * co, -beta * so);
        const double2 A12 = make_double2(alpha * co, -alpha * so), A21 = make_double2(alpha * co, alpha * so);
        double2 fh, lh;
        if (null_mode && q == 0) {                               // singular: pin l̂ = 0 (compatibility: Σ rhs = 0), shift to zero mean below
            const double d2 = A11.x * A11.x + A11.y * A11.y;
            fh = make_double2((yF.x * A11.x + yF.y * A11.y) / d2, (yF.y * A11.x - yF.x * A11.y) / d2);
            lh = make_double2(0.0, 0.0);
        } else {
            const double2 det = make_double2((A11.x * A22.x - A11.y * A22.y) - (A12.x * A21.x - A12.y * A21.y),
                                             (A11.x * A22.y + A11.y * A22.x) - (A12.x * A21.y + A12.y * A21.x));
            const double d2 = det.x * det.x + det.y * det.y;
            const double2 nf = make_double2((A22.x * yF.x - A22.y * yF.y) - (A12.x * yL.x - A12.y * yL.y),
                                            (A22.x * yF.y + A22.y * yF.x) - (A12.x * yL.y + A12.y * yL.x));
            const double2 nl = make_double2((A11.x * yL.x - A11.y * yL.y) - (A21.x * yF.x - A21.y * yF.y),
                                            (A11.x * yL.y + A11.y * yL.x) - (A21.x * yF.y + A21.y * yF.x));
            fh = make_double2((nf.x * det.x + nf.y * det.y) / d2, (nf.y * det.x - nf.x * det.y) / d2);
            lh = make_double2((nl.x * det.x + nl.y * det.y) / d2, (nl.y * det.x - nl.x * det.y) / d2);
        }
        // inverse DFT at the two rank indices this rank needs
        double s1, c1, s2, c2;
        sincospi(2.0 * (double)((q * rl) % R) / (double)R, &s1, &c1);
        sincospi(2.0 * (double)((q * rr) % R) / (double)R, &s2, &c2);
        gl.x += (lh.x * c1 - lh.y * s1) / R; gl.y += (lh.x * s1 + lh.y * c1) / R;
        gr.x += (fh.x * c2 - fh.y * s2) / R; gr.y += (fh.x * s2 + fh.y * c2) / R;
        if (null_mode) {
            // Σ_r (gL_r + gR_r) = R (l̂_0 + f̂_0): only q = 0 survives the sum over ranks
            if (q == 0) { mean.x = fh.x + lh.x; mean.y = fh.y + lh.y; }
        }
    }
    out[m] = gl;
    out[M + m] = gr;
    if (m == 0) {
        double2 mu = make_double2(0.0, 0.0);
        if (null_mode) {
            // global sum of p = Σ_r Σ_i y_r[i] - a (Σ_r gL_r + Σ_r gR_r) Σ_i s[i];  Σ_r gL_r = l̂_0, Σ_r gR_r = f̂_0 (q = 0 of the DFT)
            double2 ysum = make_double2(0.0, 0.0);
            for (int r = 0; r < R; ++r) { ysum.x += gathered[r * stride + 2 * M].x; ysum.y += gathered[r * stride + 2 * M].y; }
            const double ssum = *ssum0;
            const double cnt = (double)R * (double)N;
            mu = make_double2((ysum.x - a * mean.x * ssum) / cnt, (ysum.y - a * mean.y * ssum) / cnt);
        }
        out[2 * M] = mu;
    }
}

// p = (y - a gL s - a gR s[N-1-i] - mean[mode 0]) * scale, transposed back to the paired (ih, k, j) layout with the upper half of
// the spectrum rebuilt from the conjugate symmetry (see dist_combine_backward_kernel)
__global__ void __launch_bounds__(256) sub_correct_combine_kernel(const double2 *Y, const double *svec, const double2 *iface, double2 *Z,
                                                                  int Nxl, int Nxh, int Ny, int Nyh, int Nz, double a, double scale) {
    __shared__ double2 tA[16][17], tB[16][17];
    const int k = blockIdx.z, tx = threadIdx.x, ty = threadIdx.y;
    const long M = (long)Nyh * Nz;
    {
        const int j = blockIdx.y * 16 + tx, ih = blockIdx.x * 16 + ty;
        if (ih < Nxh && j < Nyh) {
            const long m = j + (long)Nyh * k;
            const double2 gl = iface[m], gr = iface[M + m];
            const double2 mu = m == 0 ? iface[2 * M] : make_double2(0.0, 0.0);
            double2 v[2];
#pragma unroll
            for (int o = 0; o < 2; ++o) {
                const int i = 2 * ih + o;
                if (i < Nxl) {
                    const double2 y = Y[m + M * i];
                    const double s0 = svec[m + M * i], s1 = svec[m + M * (Nxl - 1 - i)];
                    v[o] = make_double2((y.x - a * gl.x * s0 - a * gr.x * s1 - mu.x) * scale, (y.y - a * gl.y * s0 - a * gr.y * s1 - mu.y) * scale);
                } else v[o] = make_double2(0.0, 0.0);
            }
            tA[tx][ty] = v[0];
            tB[tx][ty] = v[1];
        }
    }
    __syncthreads();
    {
        const int ih = blockIdx.x * 16 + tx, j = blockIdx.y * 16 + ty;
        if (ih < Nxh && j < Nyh) {
            const double2 A = tA[ty][tx], B = tB[ty][tx];
            Z[ih + (long)Nxh * (k + (long)Nz * j)] = make_double2(A.x - B.y, A.y + B.x);
            const int jm = Ny - j, km = k == 0 ? 0 : Nz - k;
            if (j != 0 && jm >= Nyh) Z[ih + (long)Nxh * (km + (long)Nz * jm)] = make_double2(A.x + B.y, B.x - A.y);
        }
    }
}

// z-fastest variant of the local stage (R2C along z, then y): p = (y - a gL s - a gR s[N-1-i] - mean[mode 0]) * scale, in place on
// Y[kz + Nzh*(i + N*ky)]; one thread per element, mode m = kz + Nzh*ky
__global__ void __launch_bounds__(256) sub_correct_zfast_kernel(double2 *Y, const double *svec, const double2 *iface, long M, int N, int Nzh,
                                                                int Ny, double a, double scale, int Nzp) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;          // index into the padded array (pitch Nzp)
    if (t >= (long)Nzp * N * Ny) return;
    const int kz = t % Nzp;
    if (kz >= Nzh) return;                                                 // padding
    const long r = t / Nzp;
    const int i = r % N, ky = r / N;
    const long m = kz + (long)Nzh * ky;
    const double2 gl = iface[m], gr = iface[M + m];
    const double2 mu = m == 0 ? iface[2 * M] : make_double2(0.0, 0.0);
    const double2 y = Y[t];
    const double s0 = svec[m + M * i], s1 = svec[m + M * (N - 1 - i)];
    Y[t] = make_double2((y.x - a * gl.x * s0 - a * gr.x * s1 - mu.x) * scale, (y.y - a * gl.y * s0 - a * gr.y * s1 - mu.y) * scale);
    (void)Ny;
}

// ---------------------------------------------------------------------------------------------------------------------
// Round 3: the substructured x solve in the FIELDS' OWN layout (x fastest) -- "xfast". The z-fastest variant above pays for its layout
// twice: the source term and the solution are transposed through LDS (the solution a second time when the pressure correction reads it),
// and the Thomas sweeps along x touch the spectrum twice in each direction. Here nothing is transposed:
//   real rhs / solution  r[(i-1) + Nx ((j-1) + Ny (k-1))]           (what source_term_kernel<real> writes, what the dense correction reads)
//   spectrum             S[i + Nx (ky + Ny kz)],  kz = 0 .. Nz/2      (x lines contiguous: 4 KB at Nx = 256)
// * z: the real-to-complex transform of TWO neighbouring x columns at once -- (r[2i'], r[2i'+1]) read as one complex number, a complex
//   radix-4 line FFT along z in LDS (the machinery of strided_line_fft_kernel: ZL pairs = ZL x 16 B rows per workgroup), and the two
//   columns' half spectra separated with the Hermitian symmetry WHILE THE LINE IS IN LDS (paired_zline_r2c_kernel / _c2r_kernel,
//   ocn_line_fft.h);
// * y: strided_line_fft_kernel, as on the single-GPU path;
// * x: one WAVE per line. A lane holds E consecutive elements; the two Thomas recurrences f_i = (r_i - a f_{i-1}) d_i and
//   y_i = f_i - a d_i y_{i+1} are affine maps, composed across the 64 lanes by a shuffle scan (6 steps), then re-evaluated inside the lane
//   with the carried-in value -- the whole solve on ONE read of the line. The payload pass (first / last value per mode) reads only; the
//   solve pass after the all-gather runs the same kernel on the right-hand side with the interface values in its two end entries
//   (T p = r - a gL e_0 - a gR e_{N-1}) and writes the final solution: no correction pass, no s = T^-1 e_0 array.
// Same solution as the z-fastest variant to round-off (the scan re-associates the recurrences); validated at creation and by the
// partitioned-vs-single-GPU tests at 1e-12.
// ---------------------------------------------------------------------------------------------------------------------
// Thomas factors of every mode in the x-fastest layout: rden[i + N m] = 1 / (b_m - a cp[i-1]), cp = a rden (the recurrences of
// sub_setup_kernel), and of s = T^-1 e_0 only what the interface system needs: its first and last entry (and its sum for the null mode).
// `scratch` (N M doubles) holds s while it is back-substituted. One thread per mode; runs once.
__global__ void __launch_bounds__(256) sub_setup_xfast_kernel(long M, int n0, int N, double a, const double *l0, const double *l1, double *rden,
                                                              double *s_first, double *s_last, double *ssum0, double *scratch) {
    const long m = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const double b = -2.0 * a - (l0[m % n0] + l1[m / n0]);
    double *rd = rden + (long)N * m, *sv = scratch + (long)N * m;
    double c = 0.0;
    for (int i = 0; i < N; ++i) {
        const double r = 1.0 / (b - a * c);
        c = a * r;
        rd[i] = r;
    }
    double y = rd[0];
    sv[0] = y;
    for (int i = 1; i < N; ++i) { y = (-a * y) * rd[i]; sv[i] = y; }
    for (int i = N - 2; i >= 0; --i) sv[i] -= (a * rd[i]) * sv[i + 1];
    s_first[m] = sv[0];
    s_last[m] = sv[N - 1];
    if (m == 0) {
        double t = 0.0;
        for (int i = 0; i < N; ++i) t += sv[i];
        *ssum0 = t;
    }
}

// W lanes per x line (mode m; W = 64: one wave per line, W = 8 / 16 / 32: the 8 / 4 / 2 lines of a wave for the short lines of thin slabs --
// with one element per lane a 64-point line spent its time in the six scan steps: 0.115 ms per pass on a 64 x 512 x 512 slab): the Dirichlet
// solve y = T^-1 r by Thomas, both recurrences as shuffle scans of affine maps over the W lanes (see the section comment).
// SOLVE = false: reads only, payload[m] = y[0], payload[M + m] = y[N-1], payload[2M] = sum_i y[i] of mode 0.
// SOLVE = true: r_0 -= a gL, r_{N-1} -= a gR (iface[m], iface[M + m]) first, writes (y - mean[mode 0]) * scale in place.
template <int E, bool SOLVE, int W = 64>
__global__ void __launch_bounds__(256) xline_thomas_kernel(double2 *S, const double *__restrict__ rden, long M, int N, double a, double2 *payload,
                                                           const double2 *__restrict__ iface, double scale) {
    constexpr int LPW = 64 / W;                        // lines per wave
    const int lane = threadIdx.x & 63, sl = lane & (W - 1);
    const long mw = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * LPW;
    if (mw >= M) return;                               // whole waves leave together
    const long mr = mw + lane / W;
    const bool live = mr < M;                          // lines beyond the last one: lanes repeat the last line, write nothing
    const long m = live ? mr : M - 1;
    const int i0 = sl * E;
    double2 *line = S + (long)N * m;
    const double *dl = rden + (long)N * m;
    double2 r[E], f[E];
    double d[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const bool in = i0 + e < N;
        r[e] = in ? line[i0 + e] : make_double2(0.0, 0.0);
        d[e] = in ? dl[i0 + e] : 0.0;                  // beyond the line: both maps are the zero map
    }
    if (SOLVE) {
        const double2 gl = iface[m], gr = iface[M + m];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            if (i0 + e == 0) { r[e].x -= a * gl.x; r[e].y -= a * gl.y; }
            if (i0 + e == N - 1) { r[e].x -= a * gr.x; r[e].y -= a * gr.y; }
        }
    }
    // forward: f_i = A_i f_{i-1} + B_i, A_i = -a d_i, B_i = r_i d_i
    double A = 1.0, Bx = 0.0, By = 0.0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const double Ae = -a * d[e];
        Bx = Ae * Bx + r[e].x * d[e]; By = Ae * By + r[e].y * d[e];
        A = Ae * A;
    }
#pragma unroll
    for (int off = 1; off < W; off <<= 1) {
        const double Ap = __shfl_up(A, off, W), Bpx = __shfl_up(Bx, off, W), Bpy = __shfl_up(By, off, W);
        if (sl >= off) { Bx = A * Bpx + Bx; By = A * Bpy + By; A = A * Ap; }
    }
    double2 prev = make_double2(__shfl_up(Bx, 1, W), __shfl_up(By, 1, W));
    if (sl == 0) prev = make_double2(0.0, 0.0);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        f[e] = make_double2((r[e].x - a * prev.x) * d[e], (r[e].y - a * prev.y) * d[e]);
        prev = f[e];
    }
    // backward: y_i = f_i - (a d_i) y_{i+1}
    A = 1.0; Bx = 0.0; By = 0.0;
#pragma unroll
    for (int e = E - 1; e >= 0; --e) {
        const double Ae = -(a * d[e]);
        Bx = Ae * Bx + f[e].x; By = Ae * By + f[e].y;
        A = Ae * A;
    }
#pragma unroll
    for (int off = 1; off < W; off <<= 1) {
        const double Ap = __shfl_down(A, off, W), Bpx = __shfl_down(Bx, off, W), Bpy = __shfl_down(By, off, W);
        if (sl + off < W) { Bx = A * Bpx + Bx; By = A * Bpy + By; A = A * Ap; }
    }
    prev = make_double2(__shfl_down(Bx, 1, W), __shfl_down(By, 1, W));
    if (sl == W - 1) prev = make_double2(0.0, 0.0);
#pragma unroll
    for (int e = E - 1; e >= 0; --e) {
        const double c = a * d[e];
        f[e] = make_double2(f[e].x - c * prev.x, f[e].y - c * prev.y);       // f now holds y
        prev = f[e];
    }
    if (SOLVE) {
        const double2 mu = m == 0 ? iface[2 * M] : make_double2(0.0, 0.0);
#pragma unroll
        for (int e = 0; e < E; ++e)
            if (live && i0 + e < N) line[i0 + e] = make_double2((f[e].x - mu.x) * scale, (f[e].y - mu.y) * scale);
    } else {
#pragma unroll
        for (int e = 0; e < E; ++e) {
            if (live && i0 + e == 0) payload[m] = f[e];
            if (live && i0 + e == N - 1) payload[M + m] = f[e];
        }
        if (mw == 0) {                                 // the wave that holds mode 0 (its first W lanes): the sum over that line
            double sx = 0.0, sy = 0.0;
#pragma unroll
            for (int e = 0; e < E; ++e) { sx += f[e].x; sy += f[e].y; }        // entries beyond the line are zero
            for (int off = W / 2; off > 0; off >>= 1) { sx += __shfl_down(sx, off, W); sy += __shfl_down(sy, off, W); }
            if (lane == 0) payload[2 * M] = make_double2(sx, sy);
        }
    }
}

// known-answer check of the paired z transform at solver creation: pair c, level k holds (cos(2 pi k / N), sin(2 pi 3 k / N)) scaled by
// a pair-dependent amplitude; expected: X_even[1] = amp N/2, X_odd[3] = -i amp N/2, zero elsewhere (N >= 8; sampled on 256 pairs)
__device__ __forceinline__ double xfast_kat_amp(long c) { return 1.0 + 0.25 * (double)(c % 7); }
__global__ void __launch_bounds__(256) xfast_kat_fill_kernel(double2 *rp, long C, int N) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= C * N) return;
    const long c = t % C;
    const int k = (int)(t / C);
    double s3, c3, s5, c5;
    sincospi(2.0 * 1.0 * (double)k / (double)N, &s3, &c3);
    sincospi(2.0 * 3.0 * (double)k / (double)N, &s5, &c5);
    (void)s3; (void)c5;
    rp[t] = make_double2(xfast_kat_amp(c) * c3, xfast_kat_amp(c) * s5);
}
__global__ void __launch_bounds__(256) xfast_kat_check_kernel(const double2 *spec, long C, int N, double *out) {
    __shared__ double sm[256];
    const long c = (C - 1) * (long)threadIdx.x / 255;               // 256 pairs spread over the array
    double worst = 0.0;
    for (int kz = 0; kz <= N / 2; ++kz) {
        const double2 E = spec[2 * c + 2 * C * (long)kz], O = spec[2 * c + 1 + 2 * C * (long)kz];
        const double amp = xfast_kat_amp(c);
        const double2 eE = kz == 1 ? make_double2(amp * N / 2.0, 0.0) : make_double2(0.0, 0.0);
        const double2 eO = kz == 3 ? make_double2(0.0, -amp * N / 2.0) : make_double2(0.0, 0.0);
        worst = fmax(worst, fmax(fmax(fabs(E.x - eE.x), fabs(E.y - eE.y)), fmax(fabs(O.x - eO.x), fabs(O.y - eO.y))));
    }
    sm[threadIdx.x] = worst;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sm[threadIdx.x] = fmax(sm[threadIdx.x], sm[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = sm[0];
}
__global__ void __launch_bounds__(256) xfast_kat_check_real_kernel(const double2 *rp, long C, int N, double *out) {
    __shared__ double sm[256];
    const long c = (C - 1) * (long)threadIdx.x / 255;
    double worst = 0.0;
    for (int k = 0; k < N; ++k) {
        double s3, c3, s5, c5;
        sincospi(2.0 * 1.0 * (double)k / (double)N, &s3, &c3);
        sincospi(2.0 * 3.0 * (double)k / (double)N, &s5, &c5);
        (void)s3; (void)c5;
        const double2 v = rp[c + C * (long)k];
        worst = fmax(worst, fmax(fabs(v.x - xfast_kat_amp(c) * c3), fabs(v.y - xfast_kat_amp(c) * s5)));
    }
    sm[threadIdx.x] = worst;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sm[threadIdx.x] = fmax(sm[threadIdx.x], sm[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = sm[0];
}

// per-block max |a - b| (plan cross-checks)
__global__ void __launch_bounds__(256) max_abs_diff_kernel(const double *a, const double *b, long n, double *blockmax) {
    __shared__ double sm[256];
    double m = 0;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (long)gridDim.x * blockDim.x) m = fmax(m, fabs(a[q] - b[q]));
    sm[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sm[threadIdx.x] = fmax(sm[threadIdx.x], sm[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) blockmax[blockIdx.x] = sm[0];
}

// the same for two row-major complex arrays of `n0` columns and `rows` rows with different row pitches
__global__ void __launch_bounds__(256) max_abs_diff_pitched_kernel(const double2 *a, int pa, const double2 *b, int pb, int n0, long rows,
                                                                   double *blockmax) {
    __shared__ double sm[256];
    double m = 0;
    const long total = (long)n0 * rows;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
        const long r = q / n0;
        const int c = q - r * n0;
        const double2 x = a[c + (long)pa * r], y = b[c + (long)pb * r];
        m = fmax(m, fmax(fabs(x.x - y.x), fabs(x.y - y.y)));
    }
    sm[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sm[threadIdx.x] = fmax(sm[threadIdx.x], sm[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) blockmax[blockIdx.x] = sm[0];
}

// deterministic two-stage sum of a complex array (for mean(ϕ)); stage 1: per-block partials, stage 2: one block.
__global__ void __launch_bounds__(256) sum_partial_kernel(const double2 *x, long n, double2 *partial) {
    __shared__ double sx[256], sy[256];
    double ax = 0, ay = 0;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (long)gridDim.x * blockDim.x) {
        ax += x[q].x; ay += x[q].y;
    }
    sx[threadIdx.x] = ax; sy[threadIdx.x] = ay;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) { sx[threadIdx.x] += sx[threadIdx.x + s]; sy[threadIdx.x] += sy[threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = make_double2(sx[0], sy[0]);
}
__global__ void __launch_bounds__(256) sum_final_kernel(const double2 *partial, int nb, double inv_count, double scale, double2 *mean) {
    __shared__ double sx[256], sy[256];
    double ax = 0, ay = 0;
    for (int q = threadIdx.x; q < nb; q += 256) { ax += partial[q].x; ay += partial[q].y; }
    sx[threadIdx.x] = ax; sy[threadIdx.x] = ay;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) { sx[threadIdx.x] += sx[threadIdx.x + s]; sy[threadIdx.x] += sy[threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) *mean = make_double2(sx[0] * scale * inv_count, sy[0] * scale * inv_count);
}

// max |∇·u| (test helper)
__global__ void __launch_bounds__(256) max_abs_div_kernel(DGrid g, FView u, FView v, FView w, double *blockmax) {
    __shared__ double sm[256];
    double m = 0;
    long total = (long)g.Nx * g.Ny * g.Nz;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
        int i = 1 + q % g.Nx, j = 1 + (q / g.Nx) % g.Ny, k = 1 + q / ((long)g.Nx * g.Ny);
        const int kk = k - 1 + g.Hz;
        double dx = g.tx == OCN_FLAT ? 0.0 : g.ax[kk] * u.at(i + 1, j, k) - g.ax[kk] * u.at(i, j, k);
        double dy = g.ty == OCN_FLAT ? 0.0 : g.ay[kk] * v.at(i, j + 1, k) - g.ay[kk] * v.at(i, j, k);
        double dz = g.tz == OCN_FLAT ? 0.0 : g.az * w.at(i, j, k + 1) - g.az * w.at(i, j, k);
        double d = fabs(g.vinv_c[kk] * ((dx + dy) + dz));
        m = d > m ? d : m;
    }
    sm[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sm[threadIdx.x] = fmax(sm[threadIdx.x], sm[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) blockmax[blockIdx.x] = sm[0];
}

// cell_advection_timescale (Advection/cell_advection_timescale.jl:13-34): per-block maximum of the inverse timescale
// |u| Δx⁻¹ + |v| Δy⁻¹ + |w| Δzᶠ⁻¹ (min of 1/x = 1 / max of x: the division is monotone, the result has the reference's bits)
__global__ void __launch_bounds__(256) advection_timescale_kernel(DGrid g, FView u, FView v, FView w, double *blockmax) {
    __shared__ double sm[256];
    double m = 0;
    const long total = (long)g.Nx * g.Ny * g.Nz;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
        const int i = 1 + q % g.Nx, j = 1 + (q / g.Nx) % g.Ny, k = 1 + q / ((long)g.Nx * g.Ny);
        const double ix = g.tx == OCN_FLAT ? 0.0 : fabs(u.at(i, j, k)) * (1.0 / g.dx);
        const double iy = g.ty == OCN_FLAT ? 0.0 : fabs(v.at(i, j, k)) * (1.0 / g.dy);
        const double iz = g.tz == OCN_FLAT ? 0.0 : fabs(w.at(i, j, k)) * (1.0 / g.dzf[k - 1 + g.Hz]);
        const double d = (ix + iy) + iz;
        m = d > m ? d : m;
    }
    sm[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sm[threadIdx.x] = fmax(sm[threadIdx.x], sm[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) blockmax[blockIdx.x] = sm[0];
}

// hasnan(field) = any(isnan, parent(field)) (Diagnostics/nan_checker.jl:32)
__global__ void __launch_bounds__(256) hasnan_kernel(const double *a, long n, int *flag) {
    bool found = false;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (long)gridDim.x * blockDim.x) found |= a[q] != a[q];
    if (__any(found) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

// exhaustive check of rcp_rn_f32<VARIANT> against the compiler's correctly rounded divide over one binade
template <int VARIANT>
__global__ void __launch_bounds__(256) rcp_check_kernel(int exponent_bits, unsigned long long *mismatches) {
    unsigned m = blockIdx.x * blockDim.x + threadIdx.x;          // 2^23 significands
    if (m >= (1u << 23)) return;
    float x = __uint_as_float(((unsigned)exponent_bits << 23) | m);
    float a = rcp_rn_f32<VARIANT>(x), b = 1.0f / x;
    if (__float_as_uint(a) != __float_as_uint(b)) atomicAdd(mismatches, 1ULL);
}

// sampled check of rcp_rn_f64 against the compiler's IEEE divide: pseudo-random significands, exponents exp_lo..exp_hi
__global__ void __launch_bounds__(256) rcp64_check_kernel(unsigned long long n, int exp_lo, int exp_hi, unsigned long long seed,
                                                          unsigned long long *mismatches) {
    const unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    unsigned long long h = (t + seed) * 0x9E3779B97F4A7C15ull;
    h ^= h >> 31; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 29; h *= 0x94D049BB133111EBull; h ^= h >> 32;
    const unsigned long long mant = h & ((1ull << 52) - 1);
    const int e = exp_lo + (int)((h >> 52) % (unsigned long long)(exp_hi - exp_lo + 1));
    const double x = __longlong_as_double((long long)(((unsigned long long)(e + 1023) << 52) | mant));
    const double a = rcp_rn_f64(x), b = 1.0 / x;
    if (__double_as_longlong(a) != __double_as_longlong(b)) atomicAdd(mismatches, 1ULL);
}

// ---------------------------------------------------------------------------------------------------------------------
// distributed pressure solve (src/DistributedComputations)
// ---------------------------------------------------------------------------------------------------------------------
// transpose staging for the distributed FFT (distributed_transpose.jl:25-95), x-slab partition over R ranks:
//   y->x pack : zfield (Nxl, Ny, Nz)   -> send chunk d = { (i, jl, k) : j = d*Nyl + jl },  chunk-major
//   y->x unpack: recv chunk s          -> xfield (Nxg, Nyl, Nz) at i_g = s*Nxl + i
// and the inverse pair. dir 0: zfield -> chunks; 1: chunks -> xfield; 2: xfield -> chunks; 3: chunks -> zfield
__global__ void __launch_bounds__(256) transpose_stage_kernel(int dir, int R, int Nxl, int Nyl, int Nz, const double2 *src,
                                                              double2 *dst) {
    const long chunk = (long)Nxl * Nyl * Nz;
    long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= chunk * R) return;
    const int c = t / chunk;                   // peer rank index
    long q = t % chunk;
    const int i = q % Nxl;
    const int jl = (q / Nxl) % Nyl;
    const int k = q / ((long)Nxl * Nyl);
    const long Ny = (long)Nyl * R, Nxg = (long)Nxl * R;
    const long zidx = i + Nxl * ((long)(c * Nyl + jl) + Ny * k);        // zfield element (i, j = c*Nyl + jl, k)
    const long xidx = ((long)c * Nxl + i) + Nxg * (jl + (long)Nyl * k);  // xfield element (i_g = c*Nxl + i, jl, k)
    if (dir == 0) dst[t] = src[zidx];
    else if (dir == 1) dst[xidx] = src[t];
    else if (dir == 2) dst[t] = src[xidx];
    else dst[zidx] = src[t];
}

// _solve_poisson_in_spectral_space! (distributed_fft_based_poisson_solver.jl:180-188) on the x-local layout
// (Nxg, Nyc, Nz): ϕ̂ = -b̂ / (λx + λy + λz), λy indexed with the rank's mode offset; zeroth mode zeroed on the rank owning
// it. `scale` folds the inverse-transform normalisation. Padding modes (j >= Ny) carry zeros and are clamped.
__global__ void __launch_bounds__(256) dist_spectral_divide_kernel(double2 *b, const double *lx, const double *ly, const double *lz,
                                                                   int Nxg, int Nyc, int Nz, int joff, int Ny, double scale) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = blockIdx.y * blockDim.y + threadIdx.y;
    const int k = blockIdx.z;
    if (i >= Nxg || j >= Nyc || k >= Nz) return;
    const long q = (long)i + (long)Nxg * (j + (long)Nyc * k);
    const int jg = min(joff + j, Ny - 1);
    double lam = (lx[i] + ly[jg]) + lz[k] - 0.0;
    double2 val = b[q];
    val.x = -(val.x * scale) / lam;
    val.y = -(val.y * scale) / lam;
    if (i == 0 && joff + j == 0 && k == 0) { val.x = 0.0; val.y = 0.0; }
    b[q] = val;
}

// Distributed real-data transforms without real-to-complex plans: the dense real right-hand side (Nxe, Nz, Ny) -- x fastest,
// then z, then y -- is read as a complex array Z of (Nxh = Nxe/2, Nz, Ny): column pair (2i', 2i'+1) = (re, im). After the
// local complex transform in (y, z) [or y only], the transforms A, B of the two real columns are separated with the
// Hermitian symmetry  A(m) = (Z(m) + conj Z(-m)) / 2,  B(m) = (Z(m) - conj Z(-m)) / 2i,  and only the modes
// j = 0 .. Ny/2 are kept: HALF the bytes of the reference's complex-to-complex transposes go over xGMI.
// Pack for transpose_y_to_x! (distributed_transpose.jl:25-95): send chunk q = modes j in [q*Nyc, (q+1)*Nyc), layout
// (i, jl, k) with i fastest. zmirror: the z direction was transformed too (mirror k -> (Nz-k) % Nz).
__global__ void __launch_bounds__(256) dist_pack_forward_kernel(const double2 *Z, double2 *send, int Nxl, int Nxh, int Ny, int Nyh,
                                                                int Nyc, int Nyp, int Nz, bool zmirror) {
    const int ih = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = blockIdx.y * blockDim.y + threadIdx.y;
    const int k = blockIdx.z;
    if (ih >= Nxh || j >= Nyp || k >= Nz) return;
    const int q = j / Nyc, jl = j - q * Nyc;
    const long base = (((long)q * Nz + k) * Nyc + jl) * Nxl + 2 * ih;
    double2 A = make_double2(0.0, 0.0), B = A;
    if (j < Nyh) {
        const int jm = j == 0 ? 0 : Ny - j, km = (zmirror && k != 0) ? Nz - k : k;
        const double2 z1 = Z[ih + (long)Nxh * (k + (long)Nz * j)];
        const double2 z2 = Z[ih + (long)Nxh * (km + (long)Nz * jm)];
        A = make_double2(0.5 * (z1.x + z2.x), 0.5 * (z1.y - z2.y));
        B = make_double2(0.5 * (z1.y + z2.y), 0.5 * (z2.x - z1.x));
    }
    send[base] = A;
    if (2 * ih + 1 < Nxl) send[base + 1] = B;
}

// Unpack after transpose_x_to_y!: rebuild Z = A + iB for ALL modes j (upper half from the conjugate symmetry)
__global__ void __launch_bounds__(256) dist_combine_backward_kernel(const double2 *recv, double2 *Z, int Nxl, int Nxh, int Ny, int Nyh,
                                                                    int Nyc, int Nz, bool zmirror) {
    const int ih = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = blockIdx.y * blockDim.y + threadIdx.y;
    const int k = blockIdx.z;
    if (ih >= Nxh || j >= Ny || k >= Nz) return;
    const bool cj = j >= Nyh;
    const int jj = cj ? Ny - j : j, kk = (cj && zmirror && k != 0) ? Nz - k : k;
    const int q = jj / Nyc, jl = jj - q * Nyc;
    const long base = (((long)q * Nz + kk) * Nyc + jl) * Nxl + 2 * ih;
    const double2 A = recv[base];
    const double2 B = (2 * ih + 1 < Nxl) ? recv[base + 1] : make_double2(0.0, 0.0);
    Z[ih + (long)Nxh * (k + (long)Nz * j)] = cj ? make_double2(A.x + B.y, B.x - A.y) : make_double2(A.x - B.y, A.y + B.x);
}

// ---------------------------------------------------------------------------------------------------------------------
// FFT plan self-check (see ocn_api.hip: verify_*): deterministic pseudo-random pattern, round trip, compare
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double selfcheck_pattern(long q) {
    unsigned h = (unsigned)(q * 2654435761u + 12345u);
    h ^= h >> 13; h *= 0x5bd1e995u; h ^= h >> 15;
    return (double)(h & 0xFFFFFu) / 1048576.0 - 0.5;
}
__global__ void __launch_bounds__(256) selfcheck_fill_real(double *x, long n) {
    long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < n) x[q] = selfcheck_pattern(q);
}
__global__ void __launch_bounds__(256) selfcheck_fill_complex(double2 *x, long n) {
    long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < n) x[q] = make_double2(selfcheck_pattern(q), selfcheck_pattern(q + n));
}
// max |out * scale - pattern| over the dense index space; `out` is either dense (P == N, H == 0) or the interior of a haloed array
__global__ void __launch_bounds__(256) selfcheck_compare_real(const double *out, int Nx, int Ny, int Nz, int Px, int Py, int Hx, int Hy,
                                                              int Hz, double scale, double *blockmax) {
    __shared__ double sm[256];
    double m = 0;
    const long n = (long)Nx * Ny * Nz;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (long)gridDim.x * blockDim.x) {
        int i = q % Nx, j = (q / Nx) % Ny, k = q / ((long)Nx * Ny);
        double v = out[(long)(i + Hx) + (long)Px * ((j + Hy) + (long)Py * (k + Hz))];
        double d = fabs(v * scale - selfcheck_pattern(q));
        m = (d > m || d != d) ? d : m;
    }
    sm[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) { double o = sm[threadIdx.x + s]; if (o > sm[threadIdx.x] || o != o) sm[threadIdx.x] = o; }
        __syncthreads();
    }
    if (threadIdx.x == 0) blockmax[blockIdx.x] = sm[0];
}
__global__ void __launch_bounds__(256) selfcheck_compare_complex(const double2 *out, long n, double scale, double *blockmax) {
    __shared__ double sm[256];
    double m = 0;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (long)gridDim.x * blockDim.x) {
        double d = fmax(fabs(out[q].x * scale - selfcheck_pattern(q)), fabs(out[q].y * scale - selfcheck_pattern(q + n)));
        m = (d > m || d != d) ? d : m;
    }
    sm[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) { double o = sm[threadIdx.x + s]; if (o > sm[threadIdx.x] || o != o) sm[threadIdx.x] = o; }
        __syncthreads();
    }
    if (threadIdx.x == 0) blockmax[blockIdx.x] = sm[0];
}
