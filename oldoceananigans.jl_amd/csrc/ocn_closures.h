// ocn_closures.h -- the turbulence closures: ScalarDiffusivity (explicit, vertically implicit, immersed, array coefficients, Prandtl),
// AnisotropicMinimumDissipation, Smagorinsky / SmagorinskyLilly and the strain code DynamicSmagorinsky borrows (ocn_dynamic_smagorinsky.h).
// Included by ocn_kernels.h between the advection kernels (F_U .. F_C) and the tendency epilogues, which call closure_divergence; the
// z-marching epilogue (ocn_epilogue_march.h) takes the point formulas and lane_next from here. Every strain, flux and flux-divergence
// expression of the closures is written once, below; the launchers are the "closures" section of ocn_api.hip.
#pragma once
#include "ocn_device.h"
#include "ocn_immersed.h"

// ---------------------------------------------------------------------------------------------------------------------
// The point formulas, on plain doubles: the only places these expressions are written. ClosureCtx evaluates them from global memory, the
// z-marching kernels from operands they hold in registers -- the same operations in the same order on the same values (the build has
// -ffp-contract=off), hence the same bits.
// ---------------------------------------------------------------------------------------------------------------------
// Σ₁₂, Σ₁₃, Σ₂₃ = 0.5 (∂a + ∂b) from the two derivatives (velocity_tracer_gradients.jl:25-46), or from their differences δ and reciprocal
// spacings: ∂ = δ * Δ⁻¹
__device__ __forceinline__ double strain_offdiag(double da, double db) { return 0.5 * (da + db); }
__device__ __forceinline__ double strain_offdiag(double da, double ra, double db, double rb) { return strain_offdiag(da * ra, db * rb); }
// viscous_flux = -2 ν Σ at the location of Σ; diffusive_flux = -κ ∂c (abstract_scalar_diffusivity_closure.jl:194-242)
__device__ __forceinline__ double viscous_flux(double K, double S) { return -(2 * (K * S)); }
__device__ __forceinline__ double diffusive_flux(double K, double dc) { return -(K * dc); }
// a tracer's coefficient under a Smagorinsky closure: the interpolated νₑ DIVIDED by the Prandtl number (smagorinsky.jl:141-143)
__device__ __forceinline__ double prandtl_coefficient(double K, double Pr) { return K / Pr; }
// ℑxyᶜᶜᵃ, ℑxzᶜᵃᶜ, ℑyzᵃᶜᶜ of a point function f(i, j, k): x (or y) first, then the second direction
template <class Fn> __device__ __forceinline__ double interp_xy(const Fn &f, int i, int j, int k) {
    return 0.5 * (0.5 * (f(i, j, k) + f(i + 1, j, k)) + 0.5 * (f(i, j + 1, k) + f(i + 1, j + 1, k)));
}
template <class Fn> __device__ __forceinline__ double interp_xz(const Fn &f, int i, int j, int k) {
    return 0.5 * (0.5 * (f(i, j, k) + f(i + 1, j, k)) + 0.5 * (f(i, j, k + 1) + f(i + 1, j, k + 1)));
}
template <class Fn> __device__ __forceinline__ double interp_yz(const Fn &f, int i, int j, int k) {
    return 0.5 * (0.5 * (f(i, j, k) + f(i, j + 1, k)) + 0.5 * (f(i, j, k + 1) + f(i, j + 1, k + 1)));
}

// ---------------------------------------------------------------------------------------------------------------------
// ScalarDiffusivity(ν, κ): isotropic, constant, explicit closure (TurbulenceClosures/closure_kernel_operators.jl:
// 22-48, abstract_scalar_diffusivity_closure.jl:194-242, velocity_tracer_gradients.jl:5-42). viscous_flux_* = -2 ν Σᵢⱼ,
// diffusive_flux_* = -κ ∂c, ∂ = δ * (1/Δ); differences along a Flat direction vanish. The kernel ADDS the closure term to a
// tendency that already holds the advective part: G = (G - ∂ⱼτᵢⱼ) + 0.0 -- the order of the terms in
// nonhydrostatic_tendency_kernel_functions.jl:91-100 -- so it composes with the fused advection kernel.
// ---------------------------------------------------------------------------------------------------------------------
// ClosureCtx{g, u, v, w} alone is the context of a strain evaluation: no coefficient, no Flat direction (the eddy-viscosity closures are refused
// on such grids). (An aggregate with defaults, not a function that returns one: that cost the kernels below up to 12 VGPRs and ~100 instructions.)
struct ClosureCtx {
    const DGrid &g;
    const FView &u, &v, &w;
    double nu = 0.0;
    bool fx = false, fy = false, fz = false;
    // the coefficient at a flux location: the number `nu`, or -- var -- the ccc array K interpolated there
    // (abstract_scalar_diffusivity_closure.jl:310-330: ν[i,j,k], ℑxyᶠᶠᵃ, ℑxzᶠᵃᶠ, ℑyzᵃᶠᶠ, ℑxᶠᵃᵃ, ℑyᵃᶠᵃ, ℑzᵃᵃᶠ)
    // (held by value: a pointer into the kernel-argument struct would push that struct to scratch memory)
    bool var = false;
    const FView &K = u;
    __device__ __forceinline__ double K_ccc(int i, int j, int k) const { return var ? K.at(i, j, k) : nu; }
    __device__ __forceinline__ double K_fcc(int i, int j, int k) const { return var ? 0.5 * (K.at(i - 1, j, k) + K.at(i, j, k)) : nu; }
    __device__ __forceinline__ double K_cfc(int i, int j, int k) const { return var ? 0.5 * (K.at(i, j - 1, k) + K.at(i, j, k)) : nu; }
    __device__ __forceinline__ double K_ccf(int i, int j, int k) const { return var ? 0.5 * (K.at(i, j, k - 1) + K.at(i, j, k)) : nu; }
    __device__ __forceinline__ double K_ffc(int i, int j, int k) const { return var ? 0.5 * (K_fcc(i, j - 1, k) + K_fcc(i, j, k)) : nu; }
    __device__ __forceinline__ double K_fcf(int i, int j, int k) const { return var ? 0.5 * (K_fcc(i, j, k - 1) + K_fcc(i, j, k)) : nu; }
    __device__ __forceinline__ double K_cff(int i, int j, int k) const { return var ? 0.5 * (K_cfc(i, j, k - 1) + K_cfc(i, j, k)) : nu; }
    __device__ __forceinline__ double dzc(int k) const { return g.dzc[k - 1 + g.Hz]; }
    __device__ __forceinline__ double dzf(int k) const { return g.dzf[k - 1 + g.Hz]; }
    // ∂ at Center-in-d (f[+1] - f[0]) and at Face-in-d (f[0] - f[-1]); `δ * Δ⁻¹` (Operators/derivative_operators.jl:20-26) with the reciprocal
    // spacings from the grid's tables: the host formed them as the same IEEE quotients 1.0 / Δ, so a look-up equals the division it replaces
    // (four FP64 divisions per thread of the one-pass epilogue, a third of its arithmetic)
    __device__ __forceinline__ double ddx_c(const FView &f, int i, int j, int k) const { return fx ? 0.0 : (f.at(i + 1, j, k) - f.at(i, j, k)) * g.rdx; }
    __device__ __forceinline__ double ddy_c(const FView &f, int i, int j, int k) const { return fy ? 0.0 : (f.at(i, j + 1, k) - f.at(i, j, k)) * g.rdy; }
    __device__ __forceinline__ double ddz_c(const FView &f, int i, int j, int k) const { return fz ? 0.0 : (f.at(i, j, k + 1) - f.at(i, j, k)) * g.rdzc[k - 1 + g.Hz]; }
    __device__ __forceinline__ double ddx_f(const FView &f, int i, int j, int k) const { return fx ? 0.0 : (f.at(i, j, k) - f.at(i - 1, j, k)) * g.rdx; }
    __device__ __forceinline__ double ddy_f(const FView &f, int i, int j, int k) const { return fy ? 0.0 : (f.at(i, j, k) - f.at(i, j - 1, k)) * g.rdy; }
    __device__ __forceinline__ double ddz_f(const FView &f, int i, int j, int k) const { return fz ? 0.0 : (f.at(i, j, k) - f.at(i, j, k - 1)) * g.rdzf[k - 1 + g.Hz]; }
    __device__ __forceinline__ double S11(int i, int j, int k) const { return ddx_c(u, i, j, k); }
    __device__ __forceinline__ double S22(int i, int j, int k) const { return ddy_c(v, i, j, k); }
    __device__ __forceinline__ double S33(int i, int j, int k) const { return ddz_c(w, i, j, k); }
    __device__ __forceinline__ double S12(int i, int j, int k) const { return strain_offdiag(ddy_f(u, i, j, k), ddx_f(v, i, j, k)); }
    __device__ __forceinline__ double S13(int i, int j, int k) const { return strain_offdiag(ddz_f(u, i, j, k), ddx_f(w, i, j, k)); }
    __device__ __forceinline__ double S23(int i, int j, int k) const { return strain_offdiag(ddz_f(v, i, j, k), ddy_f(w, i, j, k)); }
    __device__ __forceinline__ double vf11(int i, int j, int k) const { return viscous_flux(K_ccc(i, j, k), S11(i, j, k)); }
    __device__ __forceinline__ double vf22(int i, int j, int k) const { return viscous_flux(K_ccc(i, j, k), S22(i, j, k)); }
    __device__ __forceinline__ double vf33(int i, int j, int k) const { return viscous_flux(K_ccc(i, j, k), S33(i, j, k)); }
    __device__ __forceinline__ double vf12(int i, int j, int k) const { return viscous_flux(K_ffc(i, j, k), S12(i, j, k)); }
    __device__ __forceinline__ double vf13(int i, int j, int k) const { return viscous_flux(K_fcf(i, j, k), S13(i, j, k)); }
    __device__ __forceinline__ double vf23(int i, int j, int k) const { return viscous_flux(K_cff(i, j, k), S23(i, j, k)); }
};

// V⁻¹ (δx(Ax flux) + δy(Ay flux) + δz(Az flux)) of the closure for field F at (i, j, k); coef = ν (momentum) or κ (tracer c).
// PRD (tracers of a Smagorinsky closure with Pr ≠ 1, smagorinsky.jl:141-143): K is νₑ and the coefficient at a flux point is the
// interpolated νₑ DIVIDED by the Prandtl number, which `coef` then holds (interpolate, then divide)
// VI (constant coefficients, Bounded z): the explicit part of a VerticallyImplicitTimeDiscretization (abstract_scalar_diffusivity_closure.jl:
// 245-291). At the z-flux indices k == 1 | k == Nz + 1 every z flux is the explicit one; elsewhere viscous_flux_uz = -(ν ∂xᶠᶜᶠ w),
// viscous_flux_vz = -(ν ∂yᶜᶠᶠ w), viscous_flux_wz = 0 (the test applied at its own ccc index) and diffusive_flux_z = 0: implicit_step!
// (ocn_implicit_z.h) supplies the rest. The x and y fluxes are the explicit ones.
// IM: NoImm, or the ImmView of an immersed grid (ocn_immersed.h): every flux is then conditional_flux_*(i, j, k, ibg, 0, flux) at its own
// location and index (TurbulenceClosures/immersed_diffusive_fluxes.jl:27-44) -- viscous ux, vy, wz at ccc, uy = vx at ffc, uz = wx at fcf,
// vz = wy at cff; diffusive x, y, z at fcc, cfc, ccf. Constant coefficients and explicit only (the host refuses the rest on such a grid).
template <int F, bool PRD = false, bool VI = false, class IM = NoImm>
__device__ __forceinline__ double closure_divergence(const DGrid &g, const FView &u, const FView &v, const FView &w, const FView &c,
                                                     double coef, int i, int j, int k, bool var, const FView &K, const IM &im = IM()) {
    // eddy-coefficient arrays come with grids that have no Flat direction (ocn_model_set_amd): with `var` a compile-time constant the
    // three Flat tests fold away and the loads of all six face fluxes are issued together
    const ClosureCtx X{g, u, v, w, coef, var ? false : g.tx == OCN_FLAT, var ? false : g.ty == OCN_FLAT, var ? false : g.tz == OCN_FLAT, var, K};
    const double dx_ = g.dx, dy_ = g.dy;
    auto f11 = [&](int a, int b, int d) { return im.flux(IMM_CCC, a, b, d, X.vf11(a, b, d)); };
    auto f22 = [&](int a, int b, int d) { return im.flux(IMM_CCC, a, b, d, X.vf22(a, b, d)); };
    auto f33 = [&](int a, int b, int d) { return im.flux(IMM_CCC, a, b, d, X.vf33(a, b, d)); };
    auto f12 = [&](int a, int b, int d) { return im.flux(IMM_FFC, a, b, d, X.vf12(a, b, d)); };
    auto f13 = [&](int a, int b, int d) { return im.flux(IMM_FCF, a, b, d, X.vf13(a, b, d)); };
    auto f23 = [&](int a, int b, int d) { return im.flux(IMM_CFF, a, b, d, X.vf23(a, b, d)); };
    auto kap = [&](double Kq) { return PRD ? prandtl_coefficient(Kq, coef) : Kq; };
    auto qx = [&](int a, int b, int d) { return im.flux(IMM_FCC, a, b, d, diffusive_flux(kap(X.K_fcc(a, b, d)), X.ddx_f(c, a, b, d))); };
    auto qy = [&](int a, int b, int d) { return im.flux(IMM_CFC, a, b, d, diffusive_flux(kap(X.K_cfc(a, b, d)), X.ddy_f(c, a, b, d))); };
    auto qz = [&](int a, int b, int d) { return im.flux(IMM_CCF, a, b, d, diffusive_flux(kap(X.K_ccf(a, b, d)), X.ddz_f(c, a, b, d))); };
    double dx, dy, dz, vinv;
    if (F == F_U) {            // ∂ⱼ_τ₁ⱼ at fcc: Ax_qᶜᶜᶜ, Ay_qᶠᶠᶜ, Az_qᶠᶜᶠ
        vinv = g.vinv_c[k - 1 + g.Hz];
        dx = X.fx ? 0.0 : (dy_ * X.dzc(k)) * f11(i, j, k) - (dy_ * X.dzc(k)) * f11(i - 1, j, k);
        dy = X.fy ? 0.0 : (dx_ * X.dzc(k)) * f12(i, j + 1, k) - (dx_ * X.dzc(k)) * f12(i, j, k);
        if (VI) {
            const double up = ((k + 1 == 1) | (k + 1 == g.Nz + 1)) ? f13(i, j, k + 1) : diffusive_flux(X.K_fcf(i, j, k + 1), X.ddx_f(w, i, j, k + 1));
            const double lo = ((k == 1) | (k == g.Nz + 1)) ? f13(i, j, k) : diffusive_flux(X.K_fcf(i, j, k), X.ddx_f(w, i, j, k));
            dz = (dx_ * dy_) * up - (dx_ * dy_) * lo;
        } else
        dz = X.fz ? 0.0 : (dx_ * dy_) * f13(i, j, k + 1) - (dx_ * dy_) * f13(i, j, k);
    } else if (F == F_V) {     // ∂ⱼ_τ₂ⱼ at cfc: Ax_qᶠᶠᶜ, Ay_qᶜᶜᶜ, Az_qᶜᶠᶠ
        vinv = g.vinv_c[k - 1 + g.Hz];
        dx = X.fx ? 0.0 : (dy_ * X.dzc(k)) * f12(i + 1, j, k) - (dy_ * X.dzc(k)) * f12(i, j, k);
        dy = X.fy ? 0.0 : (dx_ * X.dzc(k)) * f22(i, j, k) - (dx_ * X.dzc(k)) * f22(i, j - 1, k);
        if (VI) {
            const double up = ((k + 1 == 1) | (k + 1 == g.Nz + 1)) ? f23(i, j, k + 1) : diffusive_flux(X.K_cff(i, j, k + 1), X.ddy_f(w, i, j, k + 1));
            const double lo = ((k == 1) | (k == g.Nz + 1)) ? f23(i, j, k) : diffusive_flux(X.K_cff(i, j, k), X.ddy_f(w, i, j, k));
            dz = (dx_ * dy_) * up - (dx_ * dy_) * lo;
        } else
        dz = X.fz ? 0.0 : (dx_ * dy_) * f23(i, j, k + 1) - (dx_ * dy_) * f23(i, j, k);
    } else if (F == F_W) {     // ∂ⱼ_τ₃ⱼ at ccf: Ax_qᶠᶜᶠ, Ay_qᶜᶠᶠ, Az_qᶜᶜᶜ
        vinv = g.vinv_f[k - 1 + g.Hz];
        dx = X.fx ? 0.0 : (dy_ * X.dzf(k)) * f13(i + 1, j, k) - (dy_ * X.dzf(k)) * f13(i, j, k);
        dy = X.fy ? 0.0 : (dx_ * X.dzf(k)) * f23(i, j + 1, k) - (dx_ * X.dzf(k)) * f23(i, j, k);
        if (VI) {
            const double up = ((k == 1) | (k == g.Nz + 1)) ? f33(i, j, k) : 0.0;
            const double lo = ((k - 1 == 1) | (k - 1 == g.Nz + 1)) ? f33(i, j, k - 1) : 0.0;
            dz = (dx_ * dy_) * up - (dx_ * dy_) * lo;
        } else
        dz = X.fz ? 0.0 : (dx_ * dy_) * f33(i, j, k) - (dx_ * dy_) * f33(i, j, k - 1);
    } else {                   // ∇_dot_qᶜ at ccc: Ax_qᶠᶜᶜ, Ay_qᶜᶠᶜ, Az_qᶜᶜᶠ of -(κ ∂c) (PRD comes with `var`: no Flat test is left)
        vinv = g.vinv_c[k - 1 + g.Hz];
        const double ax = dy_ * X.dzc(k), ay = dx_ * X.dzc(k), az = dx_ * dy_;
        dx = X.fx ? 0.0 : ax * qx(i + 1, j, k) - ax * qx(i, j, k);
        dy = X.fy ? 0.0 : ay * qy(i, j + 1, k) - ay * qy(i, j, k);
        if (VI) {
            const double up = ((k + 1 == 1) | (k + 1 == g.Nz + 1)) ? qz(i, j, k + 1) : 0.0;
            const double lo = ((k == 1) | (k == g.Nz + 1)) ? qz(i, j, k) : 0.0;
            dz = az * up - az * lo;
        } else
        dz = X.fz ? 0.0 : az * qz(i, j, k + 1) - az * qz(i, j, k);
    }
    return vinv * ((dx + dy) + dz);
}

template <int F, bool VI = false, class IM = NoImm>      // IM = ImmView: the explicit constant-coefficient closure on an immersed grid
__global__ void __launch_bounds__(256) closure_tendency_kernel(DGrid g, FView u, FView v, FView w, FView c, FView G, double coef, Range6 r,
                                                               bool var, FView K, IM im) {
    const int i = r.i0 + blockIdx.x * blockDim.x + threadIdx.x;
    const int j = r.j0 + blockIdx.y * blockDim.y + threadIdx.y;
    const int k = r.k0 + blockIdx.z;
    if (i > r.i1 || j > r.j1 || k > r.k1) return;
    G.at(i, j, k) = (G.at(i, j, k) - closure_divergence<F, false, VI, IM>(g, u, v, w, c, coef, i, j, k, (VI || IM::on) ? false : var, K, im)) + 0.0;
}

// a tracer of a Smagorinsky closure with Pr ≠ 1: κ = ℑ(νₑ) / Pr at the flux points
__global__ void __launch_bounds__(256) closure_tendency_prandtl_kernel(DGrid g, FView u, FView v, FView w, FView c, FView G, double Pr, Range6 r, FView nu_e) {
    const int i = r.i0 + blockIdx.x * blockDim.x + threadIdx.x;
    const int j = r.j0 + blockIdx.y * blockDim.y + threadIdx.y;
    const int k = r.k0 + blockIdx.z;
    if (i > r.i1 || j > r.j1 || k > r.k1) return;
    G.at(i, j, k) = (G.at(i, j, k) - closure_divergence<F_C, true>(g, u, v, w, c, Pr, i, j, k, true, nu_e)) + 0.0;
}

// ---------------------------------------------------------------------------------------------------------------------
// AnisotropicMinimumDissipation(Cν, Cκ; Cb = nothing): eddy viscosity νₑ and eddy diffusivities κₑ at ccc
// (turbulence_closure_implementations/anisotropic_minimum_dissipation.jl:152-196 kernels, :226-333 terms; velocity_tracer_gradients.jl:
// 116-250 normalised gradients -- norm_∂x_u = ∂x_u unscaled, norm_∂x_v = Δᶠx/Δᶠy ∂x_v with Δᶠ = 2Δ at the CALLING index, the
// ℑxzᶜᵃᶜ of norm_∂y_w at :323 kept as written). Sums and products fold left to right, x^2 = x*x, (-C) δ² r / q.
// One thread per cell: νₑ, then κₑ of every tracer (the velocity-gradient terms are shared through the L1/L2).
// ---------------------------------------------------------------------------------------------------------------------
enum AmdOp { A_DXV, A_DYU, A_DXW, A_DZU, A_DYW, A_DZV, A_S12, A_S13, A_S23, A_DXV2, A_DYU2, A_DXW2, A_DZU2, A_DYW2, A_DZV2,
             A_DXV_S12, A_DYU_S12, A_DXW_S13, A_DZU_S13, A_DZV_S23, A_DYW_S23, A_DXC, A_DYC, A_DZC, A_DXC2, A_DYC2, A_DZC2 };
// The derived operands and the interpolations, shared by the two ways the base operands are obtained (CRTP): D::base<OP>(i, j, k)
// returns one of the twelve base operands -- the normalised gradients norm_∂x_v ... and the strain components built from them.
template <class D>
struct AmdTerms {
    __device__ __forceinline__ const D &self() const { return *static_cast<const D *>(this); }
    template <int OP> __device__ __forceinline__ double op(int i, int j, int k) const {
        switch (OP) {
        case A_DXV2: { const double x = op<A_DXV>(i, j, k); return x * x; }
        case A_DYU2: { const double x = op<A_DYU>(i, j, k); return x * x; }
        case A_DXW2: { const double x = op<A_DXW>(i, j, k); return x * x; }
        case A_DZU2: { const double x = op<A_DZU>(i, j, k); return x * x; }
        case A_DYW2: { const double x = op<A_DYW>(i, j, k); return x * x; }
        case A_DZV2: { const double x = op<A_DZV>(i, j, k); return x * x; }
        case A_DXV_S12: return op<A_DXV>(i, j, k) * op<A_S12>(i, j, k);
        case A_DYU_S12: return op<A_DYU>(i, j, k) * op<A_S12>(i, j, k);
        case A_DXW_S13: return op<A_DXW>(i, j, k) * op<A_S13>(i, j, k);
        case A_DZU_S13: return op<A_DZU>(i, j, k) * op<A_S13>(i, j, k);
        case A_DZV_S23: return op<A_DZV>(i, j, k) * op<A_S23>(i, j, k);
        case A_DYW_S23: return op<A_DYW>(i, j, k) * op<A_S23>(i, j, k);
        case A_DXC2: { const double x = op<A_DXC>(i, j, k); return x * x; }
        case A_DYC2: { const double x = op<A_DYC>(i, j, k); return x * x; }
        case A_DZC2: { const double x = op<A_DZC>(i, j, k); return x * x; }
        default: return self().template base<OP>(i, j, k);
        }
    }
    template <int OP> __device__ __forceinline__ double Ix(int i, int j, int k) const { return 0.5 * (op<OP>(i, j, k) + op<OP>(i + 1, j, k)); }
    template <int OP> __device__ __forceinline__ double Iy(int i, int j, int k) const { return 0.5 * (op<OP>(i, j, k) + op<OP>(i, j + 1, k)); }
    template <int OP> __device__ __forceinline__ double Iz(int i, int j, int k) const { return 0.5 * (op<OP>(i, j, k) + op<OP>(i, j, k + 1)); }
    template <int OP> __device__ __forceinline__ double Ixy(int i, int j, int k) const { return 0.5 * (Ix<OP>(i, j, k) + Ix<OP>(i, j + 1, k)); }
    template <int OP> __device__ __forceinline__ double Ixz(int i, int j, int k) const { return 0.5 * (Ix<OP>(i, j, k) + Ix<OP>(i, j, k + 1)); }
    template <int OP> __device__ __forceinline__ double Iyz(int i, int j, int k) const { return 0.5 * (Iy<OP>(i, j, k) + Iy<OP>(i, j, k + 1)); }
};

// metric factors and the direct evaluation of the base operands from the fields
struct AmdFields {
    const DGrid &g;
    const FView &u, &v, &w, &c;
    __device__ __forceinline__ AmdFields(const DGrid &g_, const FView &u_, const FView &v_, const FView &w_, const FView &c_) : g(g_), u(u_), v(v_), w(w_), c(c_) {}
    __device__ __forceinline__ double dzc(int k) const { return g.dzc[k - 1 + g.Hz]; }
    __device__ __forceinline__ double dzf(int k) const { return g.dzf[k - 1 + g.Hz]; }
    __device__ __forceinline__ double FX() const { return 2 * g.dx; }
    __device__ __forceinline__ double FY() const { return 2 * g.dy; }
    __device__ __forceinline__ double FZ(int k) const { return 2 * dzc(k); }
    __device__ __forceinline__ double ddx_c(const FView &f, int i, int j, int k) const { return (f.at(i + 1, j, k) - f.at(i, j, k)) * (1.0 / g.dx); }
    __device__ __forceinline__ double ddy_c(const FView &f, int i, int j, int k) const { return (f.at(i, j + 1, k) - f.at(i, j, k)) * (1.0 / g.dy); }
    __device__ __forceinline__ double ddz_c(const FView &f, int i, int j, int k) const { return (f.at(i, j, k + 1) - f.at(i, j, k)) * (1.0 / dzc(k)); }
    __device__ __forceinline__ double ddx_f(const FView &f, int i, int j, int k) const { return (f.at(i, j, k) - f.at(i - 1, j, k)) * (1.0 / g.dx); }
    __device__ __forceinline__ double ddy_f(const FView &f, int i, int j, int k) const { return (f.at(i, j, k) - f.at(i, j - 1, k)) * (1.0 / g.dy); }
    __device__ __forceinline__ double ddz_f(const FView &f, int i, int j, int k) const { return (f.at(i, j, k) - f.at(i, j, k - 1)) * (1.0 / dzf(k)); }
    template <int OP> __device__ __forceinline__ double direct(int i, int j, int k) const {
        switch (OP) {
        case A_DXV: return FX() / FY() * ddx_f(v, i, j, k);
        case A_DYU: return FY() / FX() * ddy_f(u, i, j, k);
        case A_DXW: return FX() / FZ(k) * ddx_f(w, i, j, k);
        case A_DZU: return FZ(k) / FX() * ddz_f(u, i, j, k);
        case A_DYW: return FY() / FZ(k) * ddy_f(w, i, j, k);
        case A_DZV: return FZ(k) / FY() * ddz_f(v, i, j, k);
        case A_S12: return 0.5 * (direct<A_DYU>(i, j, k) + direct<A_DXV>(i, j, k));
        case A_S13: return 0.5 * (direct<A_DZU>(i, j, k) + direct<A_DXW>(i, j, k));
        case A_S23: return 0.5 * (direct<A_DZV>(i, j, k) + direct<A_DYW>(i, j, k));
        case A_DXC: return FX() * ddx_f(c, i, j, k);
        case A_DYC: return FY() * ddy_f(c, i, j, k);
        default: return FZ(k) * ddz_f(c, i, j, k);     // A_DZC
        }
    }
    __device__ __forceinline__ double delta2(int k) const {
        const double fx = FX(), fy = FY(), fz = FZ(k);
        return 3 / ((1 / (fx * fx) + 1 / (fy * fy)) + 1 / (fz * fz));
    }
};

// every operand recomputed where it is needed (one thread per cell, no cooperation)
struct AmdCtx : AmdFields, AmdTerms<AmdCtx> {
    __device__ __forceinline__ AmdCtx(const DGrid &g_, const FView &u_, const FView &v_, const FView &w_, const FView &c_) : AmdFields(g_, u_, v_, w_, c_) {}
    template <int OP> __device__ __forceinline__ double base(int i, int j, int k) const { return direct<OP>(i, j, k); }
};

template <class A_>
__device__ __forceinline__ double amd_viscosity(const A_ &A, double Cnu, int i, int j, int k) {
    const double dxu = A.ddx_c(A.u, i, j, k), dyv = A.ddy_c(A.v, i, j, k), dzw = A.ddz_c(A.w, i, j, k);
    const double xv2 = A.template Ixy<A_DXV2>(i, j, k), yu2 = A.template Ixy<A_DYU2>(i, j, k), xw2 = A.template Ixz<A_DXW2>(i, j, k), zu2 = A.template Ixz<A_DZU2>(i, j, k),
                 yw2 = A.template Iyz<A_DYW2>(i, j, k), zv2 = A.template Iyz<A_DZV2>(i, j, k);
    double q = dxu * dxu + dyv * dyv;
    q = q + dzw * dzw;
    q = q + xv2; q = q + yu2; q = q + xw2; q = q + zu2; q = q + yw2; q = q + zv2;
    if (q == 0) return fmax(0.0, 0.0);
    double b1 = dxu * (dxu * dxu) + dyv * xv2;
    b1 = b1 + dzw * xw2;
    b1 = b1 + 2 * dxu * A.template Ixy<A_DXV_S12>(i, j, k);
    b1 = b1 + 2 * dxu * A.template Ixz<A_DXW_S13>(i, j, k);
    b1 = b1 + 2 * A.template Ixy<A_DXV>(i, j, k) * A.template Ixz<A_DXW>(i, j, k) * A.template Iyz<A_S23>(i, j, k);
    double b2 = dxu * yu2 + dyv * (dyv * dyv);
    b2 = b2 + dzw * yw2;
    b2 = b2 + 2 * dyv * A.template Ixy<A_DYU_S12>(i, j, k);
    b2 = b2 + 2 * A.template Ixy<A_DYU>(i, j, k) * A.template Iyz<A_DYW>(i, j, k) * A.template Ixz<A_S13>(i, j, k);
    b2 = b2 + 2 * dyv * A.template Iyz<A_DYW_S23>(i, j, k);
    double b3 = dxu * zu2 + dyv * zv2;
    b3 = b3 + dzw * (dzw * dzw);
    b3 = b3 + 2 * A.template Ixz<A_DZU>(i, j, k) * A.template Iyz<A_DZV>(i, j, k) * A.template Ixy<A_S12>(i, j, k);
    b3 = b3 + 2 * dzw * A.template Ixz<A_DZU_S13>(i, j, k);
    b3 = b3 + 2 * dzw * A.template Iyz<A_DZV_S23>(i, j, k);
    const double r = (b1 + b2) + b3;
    const double Cb_zeta = 0.0 / A.FZ(k);
    const double nu = -Cnu * A.delta2(k) * (r - Cb_zeta) / q;
    return fmax(0.0, nu);
}

template <class A_>
__device__ __forceinline__ double amd_diffusivity(const A_ &A, double Ck, int i, int j, int k) {
    const double xc2 = A.template Ix<A_DXC2>(i, j, k), yc2 = A.template Iy<A_DYC2>(i, j, k), zc2 = A.template Iz<A_DZC2>(i, j, k);
    const double sigma = (xc2 + yc2) + zc2;
    if (sigma == 0) return fmax(0.0, 0.0);
    const double dxu = A.ddx_c(A.u, i, j, k), dyv = A.ddy_c(A.v, i, j, k), dzw = A.ddz_c(A.w, i, j, k);
    const double cx = A.template Ix<A_DXC>(i, j, k), cy = A.template Iy<A_DYC>(i, j, k), cz = A.template Iz<A_DZC>(i, j, k);
    double t1 = dxu * xc2 + A.template Ixy<A_DXV>(i, j, k) * cx * cy;
    t1 = t1 + A.template Ixz<A_DXW>(i, j, k) * cx * cz;
    double t2 = A.template Ixy<A_DYU>(i, j, k) * cy * cx + dyv * yc2;
    t2 = t2 + A.template Ixz<A_DYW>(i, j, k) * cy * cz;
    double t3 = A.template Ixz<A_DZU>(i, j, k) * cz * cx + A.template Iyz<A_DZV>(i, j, k) * cz * cy;
    t3 = t3 + dzw * zc2;
    const double theta = (t1 + t2) + t3;
    const double kap = -Ck * A.delta2(k) * theta / sigma;
    return fmax(0.0, kap);
}

struct AmdArgs {
    int ntr;
    Range6 r;
    FView u, v, w, c[OCN_MAX_FIELDS], nu_e, kappa_e[OCN_MAX_FIELDS];
    double Cnu, Ck[OCN_MAX_FIELDS];
};

// Measured at 256 x 256 x 128 (tools/time_amd.py): 0.56 ms at 1 or 2 waves per SIMD (174 VGPRs), 0.51 ms at 3 (<= 168), 0.84 ms at 4
// (spills). Two LDS variants were built, verified bit-identical and dropped: (i) three rotating planes of u, v, w, T, S as LDS tiles
// (~10 global loads per cell instead of ~150): 0.60 ms -- the kernel is not load bound; (ii) the twelve base operands evaluated once
// per patch point and shared through LDS (~550 instead of ~1100 FP64 instructions per cell): 0.65 ms -- the ~350 LDS reads per cell
// then saturate the CU's one LDS pipe (4 clocks per wave-wide 8-byte read) and two barriers per level remain.
#ifndef OCN_AMD_WAVES
#define OCN_AMD_WAVES 3       // waves per SIMD the register allocation must allow
#endif
__global__ void __launch_bounds__(256, OCN_AMD_WAVES) amd_diffusivities_kernel(DGrid g, AmdArgs a) {
    const int i = a.r.i0 + blockIdx.x * blockDim.x + threadIdx.x;
    const int j = a.r.j0 + blockIdx.y * blockDim.y + threadIdx.y;
    const int k = a.r.k0 + blockIdx.z;
    if (i > a.r.i1 || j > a.r.j1 || k > a.r.k1) return;
    {
        const AmdCtx A(g, a.u, a.v, a.w, a.u);
        a.nu_e.at(i, j, k) = amd_viscosity(A, a.Cnu, i, j, k);
    }
#pragma unroll 1
    for (int t = 0; t < a.ntr; ++t) {
        const FView c = a.c[t], out = a.kappa_e[t];       // local copies (scalar loads): no address of a kernel argument is taken
        const AmdCtx A(g, a.u, a.v, a.w, c);
        out.at(i, j, k) = amd_diffusivity(A, a.Ck[t], i, j, k);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Round 3: the same numbers with every POINT operand evaluated once instead of up to four times. Each of the twelve base operands lives
// at a face-face-centre kind of point; a cell's doubly interpolated terms read it at 4 such points (2 for the tracer terms), which it
// shares with its neighbours -- amd_diffusivities_kernel recomputes them all (~1100 FP64 instructions per cell). Here a wave owns a
// 64-wide row of columns and MARCHES along z:
//   x: the operand of the next column is the neighbouring LANE's -- one DPP move per 32 bits (wave_shl:1), no LDS, no recomputation;
//      lane 63 only supplies its column to lane 62 (a wave writes 63 columns);
//   z: the x / y interpolated operands of level k + 1 become those of level k in the next iteration -- registers;
//   y: the thread evaluates the rows j and j + 1 itself (2x instead of 4x; no LDS, no barrier).
// The cell is then assembled by the SAME amd_viscosity / amd_diffusivity templates from a context that returns the stored interpolants,
// so every floating-point operation and its operands are those of the per-cell kernel: bit-identical (tests: == against the oracle and
// against amd_diffusivities_kernel at full size). ~350 FP64 instructions + ~60 lane moves per cell.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double lane_next(double x) {              // the value lane + 1 holds (lane 63: 0)
    int lo = __double2loint(x), hi = __double2hiint(x);
    lo = __builtin_amdgcn_update_dpp(0, lo, 0x130, 0xf, 0xf, true);   // wave_shl:1
    hi = __builtin_amdgcn_update_dpp(0, hi, 0x130, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double ix_lane(double x) { return 0.5 * (x + lane_next(x)); }      // Ix: 0.5 * (op(i) + op(i + 1))

#define OCN_AMD_MAXCHUNK 64
enum { AM_SQ1 = 0, AM_SQ2, AM_P1, AM_P2, AM_A, AM_B, AM_S, AM_N };      // per point kind: a², b², a s, b s, a, b, s = 0.5 (b + a)  [order as listed below]
template <int NTR>
struct AmdMarchCtx : AmdFields {
    // interpolants of the cell being assembled
    double ixy[AM_N];          // ffc kind: DXV2, DYU2, DXV_S12, DYU_S12, DXV, DYU, S12
    double ixz[AM_N + 1];      // fcf kind: DXW2, DZU2, DXW_S13, DZU_S13, DXW, DZU, S13; [7] = Ixz of DYW (anisotropic_minimum_dissipation.jl:323 as written)
    double iyz[AM_N];          // cff kind: DYW2, DZV2, DYW_S23, DZV_S23, DYW, DZV, S23
    double tx, tx2, ty, ty2, tz, tz2;      // tracer being assembled: Ix<DXC>, Ix<DXC2>, Iy<DYC>, Iy<DYC2>, Iz<DZC>, Iz<DZC2>
    // wave-uniform per-level factors of the cell being assembled, evaluated ONCE per block (same expressions as AmdFields::FZ / delta2 --
    // the per-cell kernel repeats these divisions in every thread: 4 per delta2, once per eddy coefficient)
    double fz_k, delta2_k;
    // ∂x u, ∂y v, ∂z w at the cell (AmdFields::ddx_c ... with their reciprocal spacings taken from the table): evaluated once, used by the
    // viscosity and by every tracer's diffusivity
    double dxu_k, dyv_k, dzw_k;
    __device__ __forceinline__ AmdMarchCtx(const DGrid &g_, const FView &u_, const FView &v_, const FView &w_) : AmdFields(g_, u_, v_, w_, u_) {}
    __device__ __forceinline__ double FZ(int) const { return fz_k; }
    __device__ __forceinline__ double delta2(int) const { return delta2_k; }
    __device__ __forceinline__ double ddx_c(const FView &, int, int, int) const { return dxu_k; }
    __device__ __forceinline__ double ddy_c(const FView &, int, int, int) const { return dyv_k; }
    __device__ __forceinline__ double ddz_c(const FView &, int, int, int) const { return dzw_k; }
    template <int OP> __device__ __forceinline__ double Ixy(int, int, int) const {
        return OP == A_DXV2 ? ixy[AM_SQ1] : OP == A_DYU2 ? ixy[AM_SQ2] : OP == A_DXV_S12 ? ixy[AM_P1] : OP == A_DYU_S12 ? ixy[AM_P2]
             : OP == A_DXV ? ixy[AM_A] : OP == A_DYU ? ixy[AM_B] : ixy[AM_S];
    }
    template <int OP> __device__ __forceinline__ double Ixz(int, int, int) const {
        return OP == A_DXW2 ? ixz[AM_SQ1] : OP == A_DZU2 ? ixz[AM_SQ2] : OP == A_DXW_S13 ? ixz[AM_P1] : OP == A_DZU_S13 ? ixz[AM_P2]
             : OP == A_DXW ? ixz[AM_A] : OP == A_DZU ? ixz[AM_B] : OP == A_S13 ? ixz[AM_S] : ixz[AM_N];
    }
    template <int OP> __device__ __forceinline__ double Iyz(int, int, int) const {
        return OP == A_DYW2 ? iyz[AM_SQ1] : OP == A_DZV2 ? iyz[AM_SQ2] : OP == A_DYW_S23 ? iyz[AM_P1] : OP == A_DZV_S23 ? iyz[AM_P2]
             : OP == A_DYW ? iyz[AM_A] : OP == A_DZV ? iyz[AM_B] : iyz[AM_S];
    }
    template <int OP> __device__ __forceinline__ double Ix(int, int, int) const { return OP == A_DXC2 ? tx2 : tx; }
    template <int OP> __device__ __forceinline__ double Iy(int, int, int) const { return OP == A_DYC2 ? ty2 : ty; }
    template <int OP> __device__ __forceinline__ double Iz(int, int, int) const { return OP == A_DZC2 ? tz2 : tz; }
};

// the seven values of a point kind from its two base operands, in AmdTerms::op's forms: a * a, b * b, a * s, b * s, a, b, s = 0.5 * (b + a)
// (S12 = 0.5 (DYU + DXV): a = DXV, b = DYU; S13 = 0.5 (DZU + DXW): a = DXW, b = DZU; S23 = 0.5 (DZV + DYW): a = DYW, b = DZV)
__device__ __forceinline__ void amd_point(double a, double b, double out[AM_N]) {
    const double s = 0.5 * (b + a);
    out[AM_SQ1] = a * a; out[AM_SQ2] = b * b; out[AM_P1] = a * s; out[AM_P2] = b * s; out[AM_A] = a; out[AM_B] = b; out[AM_S] = s;
}

#ifndef OCN_AMD_MARCH_WAVES
#define OCN_AMD_MARCH_WAVES 2       // waves per SIMD the register allocation must allow; 3 (168 VGPRs, 17 doubles spilled): 0.80 ms instead of 0.29 (measured)
#endif
#ifndef OCN_AMD_PF
#define OCN_AMD_PF 0                // levels whose loads are issued ahead of the level being evaluated (measured at 256 x 256 x 128: 2 waves per SIMD PF 0 0.249 ms,
                                    // PF 1 0.64 (256 VGPRs + spills); 1 wave per SIMD PF 1 0.286, PF 2 0.304 -- gathering the loads of a level is what pays, not their distance)
#endif
// every value a level contributes, loaded ONCE per level and ahead of its use: the loads depend on the level only, never on a result, so
// they can be issued OCN_AMD_PF levels early (measured below: no gain over gathering them at the top of their own level)
template <int NTR> struct AmdRaw {
    double uc, vc, wc;                       // u, v, w at (ic, j, L)
    double wim, wjm, wjp, vjp;               // w(ic-1, j), w(ic, j-1), w(ic, j+1), v(ic, j+1)
    double ujp, ujm, uip, vim, vimjp;        // u(ic, j+1), u(ic, j-1), u(ic+1, j), v(ic-1, j), v(ic-1, j+1)
    double c[NTR > 0 ? NTR : 1], cim[NTR > 0 ? NTR : 1], cjm[NTR > 0 ? NTR : 1], cjp[NTR > 0 ? NTR : 1];
};

template <int NTR>
__global__ void __launch_bounds__(256, OCN_AMD_MARCH_WAVES) amd_diffusivities_march_kernel(DGrid g, AmdArgs a, int kchunk) {
    // per-level factors of the levels kc0 .. kc1 + 1 of this block: FZ = 2 Δzᶜ, 1 / Δzᶠ, the four metric ratios of the normalised
    // gradients, δ² -- wave-uniform, ~17 FP64 divisions per cell in the per-cell kernel
    __shared__ double lev[8][OCN_AMD_MAXCHUNK + 2];
    const int lane = threadIdx.x;                                        // block (64, 4): a wave per row
    const int i = a.r.i0 + blockIdx.x * 63 + lane;
    const int j = a.r.j0 + blockIdx.y * blockDim.y + threadIdx.y;
    const int kc0 = a.r.k0 + blockIdx.z * kchunk, kc1 = min(kc0 + kchunk - 1, a.r.k1);
    AmdMarchCtx<NTR> A(g, a.u, a.v, a.w);
    const double fx = A.FX(), fy = A.FY(), rdx = 1.0 / g.dx, rdy = 1.0 / g.dy;
    for (int q = threadIdx.x + 64 * threadIdx.y; q <= kc1 + 1 - kc0; q += 256) {
        const int L = kc0 + q;
        const double fz = 2 * A.dzc(L);
        lev[0][q] = fz; lev[1][q] = 1.0 / A.dzf(L);
        lev[2][q] = fx / fz; lev[3][q] = fz / fx; lev[4][q] = fy / fz; lev[5][q] = fz / fy;
        lev[6][q] = 3 / ((1 / (fx * fx) + 1 / (fy * fy)) + 1 / (fz * fz));
        lev[7][q] = 1.0 / A.dzc(L);
    }
    __syncthreads();
    if (j > a.r.j1) return;                                              // (rows are independent from here on: no further barrier)
    const bool out_lane = lane < 63 && i <= a.r.i1;
    const int ic = min(i, a.r.i1 + 1);                                   // lanes beyond the last needed column repeat it (in bounds)
    const double fxfy = fx / fy, fyfx = fy / fx;
    const FView &u = a.u, &v = a.v, &w = a.w;
    typedef AmdRaw<NTR> Raw;

    auto load = [&](int L) {                                             // levels beyond the chunk's last needed one: that one again (unused)
        Raw r;
        L = min(L, kc1 + 1);
        r.uc = u.at(ic, j, L); r.vc = v.at(ic, j, L); r.wc = w.at(ic, j, L);
        r.wim = w.at(ic - 1, j, L); r.wjm = w.at(ic, j - 1, L); r.wjp = w.at(ic, j + 1, L); r.vjp = v.at(ic, j + 1, L);
        r.ujp = u.at(ic, j + 1, L); r.ujm = u.at(ic, j - 1, L); r.uip = u.at(ic + 1, j, L);
        r.vim = v.at(ic - 1, j, L); r.vimjp = v.at(ic - 1, j + 1, L);
#pragma unroll
        for (int t = 0; t < NTR; ++t) {
            const FView &c = a.c[t];
            r.c[t] = c.at(ic, j, L); r.cim[t] = c.at(ic - 1, j, L); r.cjm[t] = c.at(ic, j - 1, L); r.cjp[t] = c.at(ic, j + 1, L);
        }
        return r;
    };

    // level state carried from one iteration to the next (see the section comment)
    double ixy[AM_N], ix_fcf[AM_N + 1], iy_cff[AM_N];
    double t_ix[NTR > 0 ? NTR : 1], t_ix2[NTR > 0 ? NTR : 1], t_iy[NTR > 0 ? NTR : 1], t_iy2[NTR > 0 ? NTR : 1], t_z[NTR > 0 ? NTR : 1], t_z2[NTR > 0 ? NTR : 1];
    double n_fcf[AM_N + 1], n_cff[AM_N], n_z[NTR > 0 ? NTR : 1], n_z2[NTR > 0 ? NTR : 1];

    // fcf / cff kinds and the tracers' z operand at level L (what a cell needs of the level ABOVE it); r: level L, rb: level L - 1
    auto vertical = [&](int L, const Raw &r, const Raw &rb, double fcf[AM_N + 1], double cff[AM_N], double tz[], double tz2[]) {
        const int q = L - kc0;
        const double fz = lev[0][q], rdzf = lev[1][q], fxfz = lev[2][q], fzfx = lev[3][q], fyfz = lev[4][q], fzfy = lev[5][q];
        const double uc = r.uc, vc = r.vc, wc = r.wc;
        {   // (ic, j, L): DXW = FX / FZ * ∂x w, DZU = FZ / FX * ∂z u
            double p[AM_N];
            amd_point(fxfz * ((wc - r.wim) * rdx), fzfx * ((uc - rb.uc) * rdzf), p);
#pragma unroll
            for (int q = 0; q < AM_N; ++q) fcf[q] = ix_lane(p[q]);
        }
        double dyw0;
        {   // rows j and j + 1: DYW = FY / FZ * ∂y w, DZV = FZ / FY * ∂z v
            double p0[AM_N], p1[AM_N];
            const double wn = r.wjp, vn = r.vjp;
            dyw0 = fyfz * ((wc - r.wjm) * rdy);
            amd_point(dyw0, fzfy * ((vc - rb.vc) * rdzf), p0);
            amd_point(fyfz * ((wn - wc) * rdy), fzfy * ((vn - rb.vjp) * rdzf), p1);
#pragma unroll
            for (int q = 0; q < AM_N; ++q) cff[q] = 0.5 * (p0[q] + p1[q]);
        }
        fcf[AM_N] = ix_lane(dyw0);                                       // Ix of DYW at (·, j, L)
#pragma unroll
        for (int t = 0; t < NTR; ++t) {
            const double dzc = fz * ((r.c[t] - rb.c[t]) * rdzf);
            tz[t] = dzc; tz2[t] = dzc * dzc;
        }
    };
    // ffc kind and the tracers' x / y operands at level L (what a cell needs of its OWN level)
    auto horizontal = [&](const Raw &r) {
        double p0[AM_N], p1[AM_N];
        const double uc = r.uc, un = r.ujp, vc = r.vc, vn = r.vjp;
        amd_point(fxfy * ((vc - r.vim) * rdx), fyfx * ((uc - r.ujm) * rdy), p0);
        amd_point(fxfy * ((vn - r.vimjp) * rdx), fyfx * ((un - uc) * rdy), p1);
#pragma unroll
        for (int q = 0; q < AM_N; ++q) ixy[q] = 0.5 * (ix_lane(p0[q]) + ix_lane(p1[q]));
#pragma unroll
        for (int t = 0; t < NTR; ++t) {
            const double cc = r.c[t];
            const double dxc = fx * ((cc - r.cim[t]) * rdx);
            t_ix[t] = ix_lane(dxc); t_ix2[t] = ix_lane(dxc * dxc);
            const double dyc0 = fy * ((cc - r.cjm[t]) * rdy), dyc1 = fy * ((r.cjp[t] - cc) * rdy);
            t_iy[t] = 0.5 * (dyc0 + dyc1); t_iy2[t] = 0.5 * (dyc0 * dyc0 + dyc1 * dyc1);
        }
    };

    Raw r0, r1, r2, r3;
    {
        const Raw rm = load(kc0 - 1);
        r0 = load(kc0); r1 = load(kc0 + 1);
        if (OCN_AMD_PF >= 1) r2 = load(kc0 + 2);
        if (OCN_AMD_PF >= 2) r3 = load(kc0 + 3);
        vertical(kc0, r0, rm, ix_fcf, iy_cff, t_z, t_z2);
        horizontal(r0);
    }
    for (int k = kc0; k <= kc1; ++k) {
        // r0: level k, r1: level k + 1 (r2, r3: the levels after it, in flight)
        Raw rn;
        if (OCN_AMD_PF >= 1) rn = load(k + 2 + OCN_AMD_PF);
        vertical(k + 1, r1, r0, n_fcf, n_cff, n_z, n_z2);
#pragma unroll
        for (int q = 0; q < AM_N; ++q) { A.ixy[q] = ixy[q]; A.ixz[q] = 0.5 * (ix_fcf[q] + n_fcf[q]); A.iyz[q] = 0.5 * (iy_cff[q] + n_cff[q]); }
        A.ixz[AM_N] = 0.5 * (ix_fcf[AM_N] + n_fcf[AM_N]);
        A.fz_k = lev[0][k - kc0]; A.delta2_k = lev[6][k - kc0];
        A.dxu_k = (r0.uip - r0.uc) * rdx;
        A.dyv_k = (r0.vjp - r0.vc) * rdy;
        A.dzw_k = (r1.wc - r0.wc) * lev[7][k - kc0];
        if (out_lane) a.nu_e.at(i, j, k) = amd_viscosity(A, a.Cnu, i, j, k);
#pragma unroll
        for (int t = 0; t < NTR; ++t) {
            A.tx = t_ix[t]; A.tx2 = t_ix2[t]; A.ty = t_iy[t]; A.ty2 = t_iy2[t];
            A.tz = 0.5 * (t_z[t] + n_z[t]); A.tz2 = 0.5 * (t_z2[t] + n_z2[t]);
            if (out_lane) a.kappa_e[t].at(i, j, k) = amd_diffusivity(A, a.Ck[t], i, j, k);
        }
#pragma unroll
        for (int q = 0; q <= AM_N; ++q) ix_fcf[q] = n_fcf[q];
#pragma unroll
        for (int q = 0; q < AM_N; ++q) iy_cff[q] = n_cff[q];
#pragma unroll
        for (int t = 0; t < NTR; ++t) { t_z[t] = n_z[t]; t_z2[t] = n_z2[t]; }
        if (k < kc1) horizontal(r1);
        r0 = r1;
        if (OCN_AMD_PF == 0) r1 = load(k + 2);
        else if (OCN_AMD_PF == 1) { r1 = r2; r2 = rn; }
        else { r1 = r2; r2 = r3; r3 = rn; }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Smagorinsky(coefficient = C, Pr) and SmagorinskyLilly(C, Cb, Pr): the eddy viscosity νₑ at ccc
// (turbulence_closure_implementations/Smagorinskys/smagorinsky.jl:92-106 kernel, lilly_coefficient.jl:129-142 stability function,
// scale_invariant_operators.jl:10-13 ΣᵢⱼΣᵢⱼ at ccc, velocity_tracer_gradients.jl:25-46 strain components, BuoyancyFormulations/
// buoyancy_tracer.jl:16 and seawater_buoyancy.jl:219-224 ∂z_b). Restated:
//   Σ²  = ((((Σ11² + Σ22²) + Σ33²) + 2 Ixy(Σ12²)) + 2 Ixz(Σ13²)) + 2 Iyz(Σ23²)     Σ12 at ffc, Σ13 at fcf, Σ23 at cff; ∂ = δ * Δ⁻¹ as ClosureCtx;
//                                                                                  the interpolations nest like interp_xy / _xz / _yz
//   νₑ  = (cs² Δf²) sqrt(2 Σ²),  Δf² = cbrt((Δx Δy) Δzᶜ)² from the host's per-level table `df2`
//   cs² = C C                                              (constant coefficient)
//   cs² = (Σ² == 0 ? 0 : sqrt(1 - min(1, (Cb max(0, N²)) / Σ²))) (C C),  N² = 0.5 (∂z_b(k) + ∂z_b(k + 1))   (Lilly)
// The tracers' coefficient is ℑ(νₑ) / Pr at their flux points (smagorinsky.jl:141-143): closure_divergence<F_C, PRD>.
// ---------------------------------------------------------------------------------------------------------------------
struct SmagArgs {
    Range6 r;
    FView u, v, w, bT, S, nu_e;       // bT: the buoyancy tracer (BK 1) or T (BK 2); S: salinity (BK 2)
    double C, Cb, grav, alpha, beta;
    const double *df2;                // Δf² per level, indexed like the grid's tables [k - 1 + Hz]
};

// ∂z_b at ccf from the tracer differences ∂z bT, ∂z S (BK: 0 no buoyancy, 1 BuoyancyTracer, 2 linear SeawaterBuoyancy)
template <int BK> __device__ __forceinline__ double smag_dzb(const SmagArgs &a, double dz_bT, double dz_S) {
    return BK == 0 ? 0.0 : (BK == 1 ? dz_bT : a.grav * (a.alpha * dz_bT - a.beta * dz_S));
}

// what a cell is assembled from: the three diagonal strain components, the three interpolated squares and ∂z_b below and above the cell
struct SmagCell { double s11, s22, s33, ixy12, ixz13, iyz23, dzb_k, dzb_k1; };

// the strain part of a cell from the fields: every point value recomputed where it is needed (∂z_b left at 0)
__device__ __forceinline__ void smag_cell(const ClosureCtx &X, int i, int j, int k, SmagCell &c) {
    c.s11 = X.S11(i, j, k); c.s22 = X.S22(i, j, k); c.s33 = X.S33(i, j, k);
    c.ixy12 = interp_xy([&](int a, int b, int d) { const double x = X.S12(a, b, d); return x * x; }, i, j, k);
    c.ixz13 = interp_xz([&](int a, int b, int d) { const double x = X.S13(a, b, d); return x * x; }, i, j, k);
    c.iyz23 = interp_yz([&](int a, int b, int d) { const double x = X.S23(a, b, d); return x * x; }, i, j, k);
    c.dzb_k = 0.0; c.dzb_k1 = 0.0;
}

// Σ² of a cell: ΣᵢⱼΣᵢⱼᶜᶜᶜ (scale_invariant_operators.jl:10-13), also of the filtered velocities (Σ̄ᵢⱼΣ̄ᵢⱼᶜᶜᶜ, :119-122; ocn_dynamic_smagorinsky.h)
__device__ __forceinline__ double smag_strain_squared(const SmagCell &c) {
    double s2 = c.s11 * c.s11 + c.s22 * c.s22;
    s2 = s2 + c.s33 * c.s33;
    s2 = s2 + 2 * c.ixy12; s2 = s2 + 2 * c.ixz13; s2 = s2 + 2 * c.iyz23;
    return s2;
}

// the one assembly of a cell, shared by the per-cell and the marching kernel (=> bit-identical). DYN: cs² is the caller's `cs2_dyn`, the
// dynamic coefficient of the cell (dynamic_coefficient.jl:129-140), instead of C C
template <bool LILLY, bool DYN = false>
__device__ __forceinline__ double smagorinsky_viscosity(const SmagCell &c, const SmagArgs &a, double df2, double cs2_dyn = 0.0) {
    const double s2 = smag_strain_squared(c);
    double cs2 = DYN ? cs2_dyn : a.C * a.C;
    if (LILLY) {
        const double N2 = 0.5 * (c.dzb_k + c.dzb_k1);
        const double N2p = fmax(0.0, N2);
        const double sig2 = 1.0 - fmin(1.0, (a.Cb * N2p) / s2);
        cs2 = (s2 == 0 ? 0.0 : sqrt(sig2)) * cs2;            // a select: the quotient is NaN / Inf in fluid at rest and must not reach νₑ
    }
    return (cs2 * df2) * sqrt(2 * s2);
}

// (a) one thread per cell, every point value recomputed where it is needed
template <int BK, bool LILLY>
__global__ void __launch_bounds__(256) smagorinsky_viscosity_kernel(DGrid g, SmagArgs a) {
    const int i = a.r.i0 + blockIdx.x * blockDim.x + threadIdx.x;
    const int j = a.r.j0 + blockIdx.y * blockDim.y + threadIdx.y;
    const int k = a.r.k0 + blockIdx.z;
    if (i > a.r.i1 || j > a.r.j1 || k > a.r.k1) return;
    const ClosureCtx X{g, a.u, a.v, a.w};
    auto dzb = [&](int kk) { return smag_dzb<BK>(a, BK >= 1 ? X.ddz_f(a.bT, i, j, kk) : 0.0, BK == 2 ? X.ddz_f(a.S, i, j, kk) : 0.0); };
    SmagCell c;
    smag_cell(X, i, j, k, c);
    c.dzb_k = LILLY ? dzb(k) : 0.0; c.dzb_k1 = LILLY ? dzb(k + 1) : 0.0;
    a.nu_e.at(i, j, k) = smagorinsky_viscosity<LILLY>(c, a, a.df2[k - 1 + g.Hz]);
}

// (b) the z-march (the pattern of amd_diffusivities_march_kernel): a wave owns a 64-wide row and marches along z; every Σ12², Σ13², Σ23²
// point value is evaluated ONCE --
//   x: the value of the next column is the next lane's (one DPP move per 32 bits); lane 63 only supplies its column (63 columns written);
//   z: the x-interpolated Σ13², the y-interpolated Σ23² and ∂z_b of face level k + 1 stay in registers and are those of face level k
//      in the next iteration;
//   y: the thread evaluates the rows j and j + 1 itself.
// No LDS, no barrier. Block (64, 4): a wave per row. Measured at 256 x 256 x 128 (tools/time_smagorinsky.py, medians of interleaved runs): constant
// coefficient 0.097 ms against 0.108 of the per-cell kernel, Lilly + SeawaterBuoyancy 0.128 against 0.151; 76 .. 88 VGPRs, no scratch.
template <int BK, bool LILLY>
__global__ void __launch_bounds__(256) smagorinsky_viscosity_march_kernel(DGrid g, SmagArgs a, int kchunk) {
    const int lane = threadIdx.x;
    const int i = a.r.i0 + blockIdx.x * 63 + lane;
    const int j = a.r.j0 + blockIdx.y * blockDim.y + threadIdx.y;
    if (j > a.r.j1) return;                                              // rows are independent: whole waves leave
    const int kc0 = a.r.k0 + blockIdx.z * kchunk, kc1 = min(kc0 + kchunk - 1, a.r.k1);
    const bool out_lane = lane < 63 && i <= a.r.i1;
    const int ic = min(i, a.r.i1 + 1);                                   // lanes beyond the last needed column repeat it (in bounds)
    const double rdx = g.rdx, rdy = g.rdy;
    const FView &u = a.u, &v = a.v, &w = a.w;
    constexpr bool NB = LILLY && BK >= 1, NS = LILLY && BK == 2;         // which tracers are read at all
    struct Raw {
        double uc, ujm, ujp;                 // u at (ic, j), (ic, j - 1), (ic, j + 1)
        double vc, vjp, vim, vimjp;          // v at (ic, j), (ic, j + 1), (ic - 1, j), (ic - 1, j + 1)
        double wc, wim, wjm, wjp;            // w at (ic, j), (ic - 1, j), (ic, j - 1), (ic, j + 1)
        double b, s;                         // the buoyancy tracers at (ic, j)
    };
    auto load = [&](int L) {                                             // levels beyond the chunk's last needed one: that one again (unused)
        Raw r;
        L = min(L, kc1 + 1);
        r.uc = u.at(ic, j, L); r.ujm = u.at(ic, j - 1, L); r.ujp = u.at(ic, j + 1, L);
        r.vc = v.at(ic, j, L); r.vjp = v.at(ic, j + 1, L); r.vim = v.at(ic - 1, j, L); r.vimjp = v.at(ic - 1, j + 1, L);
        r.wc = w.at(ic, j, L); r.wim = w.at(ic - 1, j, L); r.wjm = w.at(ic, j - 1, L); r.wjp = w.at(ic, j + 1, L);
        r.b = NB ? a.bT.at(ic, j, L) : 0.0; r.s = NS ? a.S.at(ic, j, L) : 0.0;
        return r;
    };
    // face level L (r: level L, rb: level L - 1): Ix of Σ13² at (·, j, L), Iy of Σ23² at (i, ·, L), ∂z_b at (i, j, L)
    auto vertical = [&](int L, const Raw &r, const Raw &rb, double &ix13, double &iy23, double &dzb) {
        const double rdzf = g.rdzf[L - 1 + g.Hz];
        const double s13 = strain_offdiag(r.uc - rb.uc, rdzf, r.wc - r.wim, rdx);
        ix13 = ix_lane(s13 * s13);
        const double s23_0 = strain_offdiag(r.vc - rb.vc, rdzf, r.wc - r.wjm, rdy), s23_1 = strain_offdiag(r.vjp - rb.vjp, rdzf, r.wjp - r.wc, rdy);
        iy23 = 0.5 * (s23_0 * s23_0 + s23_1 * s23_1);
        dzb = smag_dzb<BK>(a, NB ? (r.b - rb.b) * rdzf : 0.0, NS ? (r.s - rb.s) * rdzf : 0.0);
    };
    // own level: Ixy of Σ12² (rows j and j + 1)
    auto horizontal = [&](const Raw &r) {
        const double s12_0 = strain_offdiag(r.uc - r.ujm, rdy, r.vc - r.vim, rdx), s12_1 = strain_offdiag(r.ujp - r.uc, rdy, r.vjp - r.vimjp, rdx);
        return 0.5 * (ix_lane(s12_0 * s12_0) + ix_lane(s12_1 * s12_1));
    };
    Raw r0 = load(kc0), r1 = load(kc0 + 1);
    double ix13, iy23, dzb;
    {
        const Raw rm = load(kc0 - 1);
        vertical(kc0, r0, rm, ix13, iy23, dzb);
    }
    for (int k = kc0; k <= kc1; ++k) {
        // r0: level k, r1: level k + 1
        double n13, n23, ndzb;
        vertical(k + 1, r1, r0, n13, n23, ndzb);
        SmagCell c;
        c.s11 = (lane_next(r0.uc) - r0.uc) * rdx;                        // (the next lane holds column i + 1 for every lane that writes)
        c.s22 = (r0.vjp - r0.vc) * rdy;
        c.s33 = (r1.wc - r0.wc) * g.rdzc[k - 1 + g.Hz];
        c.ixy12 = horizontal(r0);
        c.ixz13 = 0.5 * (ix13 + n13); c.iyz23 = 0.5 * (iy23 + n23);
        c.dzb_k = dzb; c.dzb_k1 = ndzb;
        if (out_lane) a.nu_e.at(i, j, k) = smagorinsky_viscosity<LILLY>(c, a, a.df2[k - 1 + g.Hz]);
        ix13 = n13; iy23 = n23; dzb = ndzb;
        r0 = r1;
        r1 = load(k + 2);
    }
}
