// ocn_dynamic_smagorinsky.h -- Smagorinsky(coefficient = DynamicCoefficient(averaging, schedule, minimum_numerator)): the scale-invariant
// dynamic procedure of Bou-Zeid et al. (2005) as the reference writes it (turbulence_closure_implementations/Smagorinskys/
// dynamic_coefficient.jl, scale_invariant_operators.jl, smagorinsky.jl:92-127). Restated:
//   filter(f)  = ((((((6 f + f[i+1]) + f[i-1]) + f[j+1]) + f[j-1]) + f[k+1]) + f[k-1]) / 12            (scale_invariant_operators.jl:47-55)
//   Σ          = sqrt(Σ²),  Σ̄ = sqrt(Σ̄²): Σ² as smag_strain_squared assembles it, Σ̄² the same of the FILTERED velocities (:62-122)
//   Lᵢⱼ        = filter(uᵢuⱼ at ccc) - ūᵢūⱼ at ccc                                                      (:161-188)
//                  u₁u₁ = ℑx(u²), ū₁ū₁ = ℑx(ū²); u₁u₂ = ℑx(u) ℑy(v), ū₁ū₂ = ℑx(ū) ℑy(v̄); ℑ(f) = 0.5 (f + f[+1])
//   Mᵢⱼ        = (2 Δf²) (filter(Σ Σᵢⱼ at ccc) - 4 (Σ̄ Σ̄ᵢⱼ at ccc))                                       (:126-159)
//                  Σ₁₂ at ccc = ℑxy(Σ₁₂), Σ₁₃ = ℑxz(Σ₁₃), Σ₂₃ = ℑyz(Σ₂₃), nested like the squares in Σ²
//   LM         = ((((L₁₁ M₁₁ + L₂₂ M₂₂) + L₃₃ M₃₃) + (2 L₁₂) M₁₂) + (2 L₁₃) M₁₃) + (2 L₂₃) M₂₃, MM likewise   (dynamic_coefficient.jl:169-188)
//   cs²        = 𝒥ᴹᴹ > 0 ? max(𝒥ᴸᴹ, minimum_numerator) / 𝒥ᴹᴹ : 0      (:129-140; `* false` is a strong zero there: a SELECT here)
// Two facts of the reference that the kernels reproduce: Σ and Σ̄ are computed over the interior and their halos are never filled, so
// filter(Σ Σᵢⱼ) reads Σ = 0 at every neighbour outside the interior, next to a Periodic boundary too (dyn_lm_mm_kernel: a select); and
// the Lagrangian 𝒥 fields get their halos once, from the initialising mean (dyn_fill_mean_kernel writes whole parent arrays; the averaging
// pass writes the interior only; the copy to 𝒥⁻ is a copy of the parent).
//
// Kernel split. The reference's call tree, one thread per cell, would evaluate the filtered velocities 30 times per cell and their strain
// from scratch. What many cells share is staged in parent-shaped arrays instead (storing an FP64 value changes no bit under
// -ffp-contract=off):
//   1 dyn_filter_sigma_kernel   ū, v̄, w̄ on the interior plus one ring (they read u, v, w to ±2: halos >= 2), Σ on the interior
//   2 dyn_sigma_bar_kernel      Σ̄ on the interior from ū, v̄, w̄
//   3 dyn_lm_mm_kernel          LM, MM: ONE walk over the cell and its six neighbours accumulates the twelve filter sums (each in the
//                               reference's order), then one Lᵢⱼ, Mᵢⱼ pair at a time is folded into LM and MM. LAGR: fused with the Lagrangian
//                               averaging update (_lagrangian_average_LM_MM!, dynamic_coefficient.jl:241-290), as the reference fuses it.
//   smagorinsky_viscosity_dynamic_kernel   νₑ with cs² read from the 𝒥 arrays (stride 0 along an averaged direction)
#pragma once
#include "ocn_kernels.h"
#include "ocn_open_boundary.h"   // jl_max
#include "ocn_particles.h"       // particle_interpolator, particle_interpolate: the reference's `interpolate`

struct DynArgs {
    FView u, v, w;               // the velocities (halos filled)
    FView ub, vb, wb;            // ū, v̄, w̄ at the locations of u, v, w (scratch)
    FView Sig, Sigb;             // Σ, Σ̄ at ccc
    FView LM, MM;                // what pass 3 writes: LM, MM (directional, and the initialising Lagrangian update) or 𝒥ᴸᴹ, 𝒥ᴹᴹ (Lagrangian)
    FView JLMp, JMMp;            // 𝒥ᴸᴹ⁻, 𝒥ᴹᴹ⁻ (Lagrangian)
    const double *df2, *df;      // Δf², Δf per level [k - 1 + Hz]
    const double *xc, *yc, *zc;  // the centre nodes [i - 1] (Lagrangian)
    double jmin, dt;             // minimum_numerator; Δt since the previous call (Lagrangian)
};

// where the νₑ kernel reads 𝒥ᴸᴹ, 𝒥ᴹᴹ: element of the 0-based interior point (i, j, k) at off + i s[0] + j s[1] + k s[2] (DgOut's layout)
struct DynCoefficient {
    const double *jlm, *jmm;
    long off, s[3];
    double jmin;
};

__device__ __forceinline__ double dyn_filter(const FView &f, int i, int j, int k) {
    double s = 6 * f.at(i, j, k) + f.at(i + 1, j, k);
    s = s + f.at(i - 1, j, k); s = s + f.at(i, j + 1, k); s = s + f.at(i, j - 1, k); s = s + f.at(i, j, k + 1); s = s + f.at(i, j, k - 1);
    return s / 12;
}

// the six strain components at ccc, in the order 11, 22, 33, 12, 13, 23 (the squares of a cell: smag_cell, ocn_closures.h)
__device__ __forceinline__ void dyn_strain(const ClosureCtx &X, int i, int j, int k, double s[6]) {
    s[0] = X.S11(i, j, k); s[1] = X.S22(i, j, k); s[2] = X.S33(i, j, k);
    s[3] = interp_xy([&](int a, int b, int d) { return X.S12(a, b, d); }, i, j, k);
    s[4] = interp_xz([&](int a, int b, int d) { return X.S13(a, b, d); }, i, j, k);
    s[5] = interp_yz([&](int a, int b, int d) { return X.S23(a, b, d); }, i, j, k);
}

__device__ __forceinline__ double dyn_sigma(const ClosureCtx &X, int i, int j, int k) {      // Σ = sqrt(Σ²) of a cell
    SmagCell c;
    smag_cell(X, i, j, k, c);
    return sqrt(smag_strain_squared(c));
}

// pass 1 over i = 0 .. Nx + 1, j = 0 .. Ny + 1, k = 0 .. Nz + 1 (_compute_Σ!, dynamic_coefficient.jl:142-149, and the filtered velocities)
__global__ void __launch_bounds__(256) dyn_filter_sigma_kernel(DGrid g, DynArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y, k = blockIdx.z;
    if (i > g.Nx + 1 || j > g.Ny + 1) return;
    a.ub.at(i, j, k) = dyn_filter(a.u, i, j, k);
    a.vb.at(i, j, k) = dyn_filter(a.v, i, j, k);
    a.wb.at(i, j, k) = dyn_filter(a.w, i, j, k);
    if (i < 1 || i > g.Nx || j < 1 || j > g.Ny || k < 1 || k > g.Nz) return;
    a.Sig.at(i, j, k) = dyn_sigma(ClosureCtx{g, a.u, a.v, a.w}, i, j, k);
}

// pass 2 over the interior (_compute_Σ̄!, dynamic_coefficient.jl:151-158)
__global__ void __launch_bounds__(256) dyn_sigma_bar_kernel(DGrid g, DynArgs a) {
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x, j = 1 + blockIdx.y * blockDim.y + threadIdx.y, k = 1 + blockIdx.z;
    if (i > g.Nx || j > g.Ny) return;
    a.Sigb.at(i, j, k) = dyn_sigma(ClosureCtx{g, a.ub, a.vb, a.wb}, i, j, k);
}

// clamp(x, lo, hi) (Base: ifelse(x > hi, hi, ifelse(x < lo, lo, x)))
__device__ __forceinline__ double dyn_clamp(double x, double lo, double hi) { return x > hi ? hi : (x < lo ? lo : x); }

// pass 3 over the interior (_compute_LM_MM!, dynamic_coefficient.jl:160-188; LAGR: _lagrangian_average_LM_MM!, :241-290)
template <bool LAGR>
__global__ void __launch_bounds__(256) dyn_lm_mm_kernel(DGrid g, DynArgs a, PGeom pg) {
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x, j = 1 + blockIdx.y * blockDim.y + threadIdx.y, k = 1 + blockIdx.z;
    if (i > g.Nx || j > g.Ny) return;
    const ClosureCtx X{g, a.u, a.v, a.w};
    // the filter sums of uᵢuⱼ (fl) and of Σ Σᵢⱼ (fm) over the cell, i + 1, i - 1, j + 1, j - 1, k + 1, k - 1 -- the order the reference adds them in
    double fl[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, fm[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
    for (int q = 0; q < 7; ++q) {
        const int ii = i + (q == 1) - (q == 2), jj = j + (q == 3) - (q == 4), kk = k + (q == 5) - (q == 6);
        const double u0 = a.u.at(ii, jj, kk), u1 = a.u.at(ii + 1, jj, kk);
        const double v0 = a.v.at(ii, jj, kk), v1 = a.v.at(ii, jj + 1, kk);
        const double w0 = a.w.at(ii, jj, kk), w1 = a.w.at(ii, jj, kk + 1);
        const double uc = 0.5 * (u0 + u1), vc = 0.5 * (v0 + v1), wc = 0.5 * (w0 + w1);
        const double t[6] = {0.5 * (u0 * u0 + u1 * u1), 0.5 * (v0 * v0 + v1 * v1), 0.5 * (w0 * w0 + w1 * w1), uc * vc, uc * wc, vc * wc};
        // Σ outside the interior is the never-filled halo of the reference's field: 0
        const bool inside = ii >= 1 && ii <= g.Nx && jj >= 1 && jj <= g.Ny && kk >= 1 && kk <= g.Nz;
        const double sig = inside ? a.Sig.at(ii, jj, kk) : 0.0;
        double s[6];
        dyn_strain(X, ii, jj, kk, s);
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const double m = sig * s[c];
            fl[c] = q == 0 ? 6 * t[c] : fl[c] + t[c];
            fm[c] = q == 0 ? 6 * m : fm[c] + m;
        }
    }
    // ūᵢūⱼ and Σ̄ Σ̄ᵢⱼ at the cell itself
    const double ub0 = a.ub.at(i, j, k), ub1 = a.ub.at(i + 1, j, k);
    const double vb0 = a.vb.at(i, j, k), vb1 = a.vb.at(i, j + 1, k);
    const double wb0 = a.wb.at(i, j, k), wb1 = a.wb.at(i, j, k + 1);
    const double ubc = 0.5 * (ub0 + ub1), vbc = 0.5 * (vb0 + vb1), wbc = 0.5 * (wb0 + wb1);
    const double tb[6] = {0.5 * (ub0 * ub0 + ub1 * ub1), 0.5 * (vb0 * vb0 + vb1 * vb1), 0.5 * (wb0 * wb0 + wb1 * wb1), ubc * vbc, ubc * wbc, vbc * wbc};
    const ClosureCtx XB{g, a.ub, a.vb, a.wb};
    double sb[6];
    dyn_strain(XB, i, j, k, sb);
    const double sigb = a.Sigb.at(i, j, k);
    const double c2 = 2 * a.df2[k - 1 + g.Hz];
    // one component at a time: L₁₁ M₁₁, L₂₂ M₂₂, L₃₃ M₃₃, (2 L₁₂) M₁₂, (2 L₁₃) M₁₃, (2 L₂₃) M₂₃
    double LM = 0.0, MM = 0.0;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        const double L = fl[c] / 12 - tb[c];
        const double M = c2 * (fm[c] / 12 - 4 * (sigb * sb[c]));
        const double lm = c < 3 ? L * M : (2 * L) * M, mm = c < 3 ? M * M : (2 * M) * M;
        LM = c == 0 ? lm : LM + lm;
        MM = c == 0 ? mm : MM + mm;
    }
    if (!LAGR) {
        a.LM.at(i, j, k) = LM;
        a.MM.at(i, j, k) = MM;
        return;
    }
    const double jl = jl_max(a.JLMp.at(i, j, k), a.jmin), jm = a.JMMp.at(i, j, k);
    const double T = (1.5 * a.df[k - 1 + g.Hz]) / sqrt(sqrt(sqrt(sqrt(jl * jm))));       // ∜(∜(x)), ∜ = sqrt ∘ sqrt (Base.fourthroot)
    const double tau = a.dt / T;
    const double eps = tau / (1 + tau);
    // the velocities at the cell's own index, not interpolated to the cell centre (:263-265); displacements of one spacing at most
    const double ddx = dyn_clamp(a.u.at(i, j, k) * a.dt, -g.dx, g.dx);
    const double ddy = dyn_clamp(a.v.at(i, j, k) * a.dt, -g.dy, g.dy);
    const double dzk = g.dzc[k - 1 + g.Hz];
    const double ddz = dyn_clamp(a.w.at(i, j, k) * a.dt, -dzk, dzk);
    const PInterp ix = particle_interpolator(pg, 0, false, a.xc[i - 1] - ddx);
    const PInterp iy = particle_interpolator(pg, 1, false, a.yc[j - 1] - ddy);
    const PInterp iz = particle_interpolator(pg, 2, false, a.zc[k - 1] - ddz);
    const double imm = particle_interpolate(a.JMMp, ix, iy, iz);
    const double ilm = particle_interpolate(a.JLMp, ix, iy, iz);
    a.MM.at(i, j, k) = eps * MM + (1 - eps) * imm;
    const double star = eps * LM + (1 - eps) * jl_max(ilm, a.jmin);
    a.LM.at(i, j, k) = jl_max(star, a.jmin);
}

// parent(𝒥) .= mean, with max(mean, minimum_numerator) where `clamped` (dynamic_coefficient.jl:320-321): the whole parent array
__global__ void __launch_bounds__(256) dyn_fill_mean_kernel(double *p, long n, const double *mean, int clamped, double jmin) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const double m = *mean;
    p[q] = clamped ? jl_max(m, jmin) : m;
}

// _compute_smagorinsky_viscosity! with the dynamic coefficient (smagorinsky.jl:92-106, dynamic_coefficient.jl:129-140) over the interior
__global__ void __launch_bounds__(256) smagorinsky_viscosity_dynamic_kernel(DGrid g, SmagArgs a, DynCoefficient d) {
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x, j = 1 + blockIdx.y * blockDim.y + threadIdx.y, k = 1 + blockIdx.z;
    if (i > g.Nx || j > g.Ny) return;
    const ClosureCtx X{g, a.u, a.v, a.w};
    SmagCell c;
    smag_cell(X, i, j, k, c);
    const long q = d.off + (i - 1) * d.s[0] + (j - 1) * d.s[1] + (k - 1) * d.s[2];
    const double jl = jl_max(d.jlm[q], d.jmin), jm = d.jmm[q];
    const double cs2 = jm > 0 ? jl / jm : 0.0;             // fluid at rest: 𝒥ᴹᴹ = 0 and the quotient Inf -- discarded, νₑ = 0
    a.nu_e.at(i, j, k) = smagorinsky_viscosity<false, true>(c, a, a.df2[k - 1 + g.Hz], cs2);
}
