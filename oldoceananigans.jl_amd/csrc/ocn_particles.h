// ocn_particles.h -- particles = LagrangianParticles of the NonhydrostaticModel: step_lagrangian_particles! as ONE launch
// (Models/LagrangianParticleTracking/LagrangianParticleTracking.jl:140-149): every tracked property is set to its field interpolated at the
// particle (update_lagrangian_particle_properties.jl:6-36), then the particle moves with the interpolated total velocities
// (lagrangian_particle_advection.jl:118-178; drogued_dynamics.jl:45-72). Trilinear interpolation as Fields/interpolate.jl:15-59,67-83,
// 137-188,272-336 writes it. Arithmetic contract of ocn_device.h: no contraction (the reference writes no @muladd in these files), a true IEEE
// division, every expression in the reference's association order.
//
// One thread per particle, structure of arrays. A thread forms the Face and the Center interpolator of each direction once (six; eight with
// drogue depths) and every field of the launch reuses them. The geometry and the field views arrive as kernel arguments; the node tables
// of a stretched z (Nz + 1 and Nz doubles) are read by the binary search through the caches. No LDS.
//
// Bounds: the reference reads @inbounds and would leave the array for a position far outside the domain or a NaN. Here every corner index is
// clamped into the parent range of its direction after the interpolator is formed (particle_interpolator), and NaN / Inf take comparisons,
// never a float -> int conversion of an unrepresentable value. The clamp changes nothing within one halo cell of the domain.
#pragma once
#include "ocn_device.h"
#include <math.h>

#define OCN_MAX_TRACKED 8

// what the index computation needs of a grid. Per direction d: N, H, topology code, the first Face and the first Center node (x₀ of
// fractional_x_index at that location), the spacing, and the walls xᴸ = face 1, xᴿ = face N + 1 of enforce_boundary_conditions.
// zf / zc: the Nz + 1 face and Nz centre nodes of a stretched z (NULL: z is regular or Flat).
struct PGeom {
    int N[3], H[3], T[3];
    double f0[3], c0[3], d[3], xL[3], xR[3];
    const double *zf, *zc;
};

struct PInterp { int lo, hi; double w; };      // (i⁻, i⁺, ξ) of interpolator (interpolate.jl:298-308)

// mod(x, y) for floats as Julia defines it (base/float.jl): rem, then the sign of y on a zero and + y where the signs differ
__host__ __device__ __forceinline__ double julia_mod(double x, double y) {
    const double r = fmod(x, y);
    if (r == 0.0) return copysign(r, y);
    if ((r > 0.0) != (y > 0.0)) return r + y;
    return r;
}

// index_binary_search + fractional_index (interpolate.jl:30-59) over the n nodes of `vec` (0-based storage of the 1-based vector)
__host__ __device__ __forceinline__ double fractional_index(double val, const double *vec, int n) {
    int low = 0, high = n - 1;
    while (low + 1 < high) {
        const int mid = (low + high) / 2;          // unsafe_trunc(Int, (l + h) / 2) of non-negative integers
        const double v = vec[mid];                 // vec[mid + 1], 1-based
        if (v == val) { low = high = mid; break; }        // return (mid + 1, mid + 1)
        else if (v < val) low = mid;
        else high = mid;
    }
    const int i1 = low + 1, i2 = high + 1;
    const double x1 = vec[i1 - 1], x2 = vec[i2 - 1];
    const double ii = (double)(i2 - i1) / (x2 - x1) * (val - x1) + (double)i1;
    return i1 == i2 ? (double)i1 : ii;
}

// The fractional index of coordinate `x` along direction d at location `face` (fractional_x/y/z_index) and its interpolator, the corner
// indices clamped into the parent range [1 - H, N + H (+ 1 for a Face that ends in a wall)]. Flat: interpolator(::Nothing) = (1, 1, 0).
__host__ __device__ __forceinline__ PInterp particle_interpolator(const PGeom &g, int d, bool face, double x) {
    PInterp r;
    if (g.T[d] == 3) { r.lo = 1; r.hi = 1; r.w = 0.0; return r; }
    double fidx;
    const double *tab = d == 2 ? (face ? g.zf : g.zc) : nullptr;
    if (tab) fidx = fractional_index(x, tab, face ? g.N[2] + 1 : g.N[2]);
    else fidx = (x - (face ? g.f0[d] : g.c0[d])) / g.d[d] + 1.0;
    const int lo = 1 - g.H[d], hi = g.N[d] + g.H[d] + ((face && wall_hi(g.T[d])) ? 1 : 0);
    const double t = trunc(fidx);
    // NaN fails both comparisons' first and lands on `lo`; ±Inf and anything beyond the parent array land on its ends
    r.lo = (t >= (double)lo) ? ((t <= (double)hi) ? (int)t : hi) : lo;
    r.hi = r.lo + 1 > hi ? hi : r.lo + 1;
    r.w = julia_mod(fidx, 1.0);
    return r;
}

// enforce_boundary_conditions (lagrangian_particle_advection.jl:10-46) by topology code: 0 Periodic, 1 Bounded, 3 Flat
__host__ __device__ __forceinline__ double particle_boundary(int topo, double x, double xL, double xR, double Cr) {
    if (topo == 1) {
        if (x > xR) { const double xi = xR - Cr * (x - xR); return xi < xL ? xL : xi; }       // bounce_left
        if (x < xL) { const double xi = xL + Cr * (xL - x); return xi > xR ? xR : xi; }       // bounce_right
        return x;
    }
    if (topo == 0) {
        if (x > xR) return xL + julia_mod(x - xR, xR - xL);
        if (x < xL) return xR - julia_mod(xL - x, xR - xL);
        return x;
    }
    return x;
}

#ifdef __HIPCC__
// _interpolate (interpolate.jl:313-336): all eight products, each ϕ a left-associated product, summed left to right, k fastest
__device__ __forceinline__ double particle_interpolate(const FView &f, const PInterp &ix, const PInterp &iy, const PInterp &iz) {
    const double xi = ix.w, eta = iy.w, zeta = iz.w;
    const double ax = 1.0 - xi, ay = 1.0 - eta, az = 1.0 - zeta;
    const long i0 = f.off + ix.lo, i1 = f.off + ix.hi;
    const long j0 = (long)f.s1 * iy.lo, j1 = (long)f.s1 * iy.hi;
    const long k0 = f.s2 * iz.lo, k1 = f.s2 * iz.hi;
    const double *p = f.p;
    double s = ((ax * ay) * az) * p[i0 + j0 + k0];
    s = s + ((ax * ay) * zeta) * p[i0 + j0 + k1];
    s = s + ((ax * eta) * az) * p[i0 + j1 + k0];
    s = s + ((ax * eta) * zeta) * p[i0 + j1 + k1];
    s = s + ((xi * ay) * az) * p[i1 + j0 + k0];
    s = s + ((xi * ay) * zeta) * p[i1 + j0 + k1];
    s = s + ((xi * eta) * az) * p[i1 + j1 + k0];
    s = s + ((xi * eta) * zeta) * p[i1 + j1 + k1];
    return s;
}

// a field at location (lx, ly, lz) (bit d of `loc`: Face) and the per-particle array its samples go to
struct TrackedField { FView f; int loc; double *out; };

struct ParticleStepArgs {
    int n;
    double *x, *y, *z;
    const double *depths;           // DroguedParticleDynamics(depths), or NULL
    double restitution, dt;
    int advect;                     // 0: sample the tracked fields only (ocn_interpolate_at)
    FView u, v, w;                  // total_velocities(model)
    int ntracked;
    TrackedField tracked[OCN_MAX_TRACKED];
};

__global__ __launch_bounds__(256) void particle_step_kernel(PGeom g, ParticleStepArgs a) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= a.n) return;
    const double x = a.x[p], y = a.y[p], z = a.z[p];
    const PInterp xc = particle_interpolator(g, 0, false, x), xf = particle_interpolator(g, 0, true, x);
    const PInterp yc = particle_interpolator(g, 1, false, y), yf = particle_interpolator(g, 1, true, y);
    const PInterp zc = particle_interpolator(g, 2, false, z), zf = particle_interpolator(g, 2, true, z);
    for (int q = 0; q < a.ntracked; ++q) {             // update_lagrangian_particle_properties!: at the position before the move
        const TrackedField &t = a.tracked[q];
        t.out[p] = particle_interpolate(t.f, (t.loc & 1) ? xf : xc, (t.loc & 2) ? yf : yc, (t.loc & 4) ? zf : zc);
    }
    if (!a.advect) return;
    PInterp ac = zc, af = zf;                          // drogued: the velocities at (x, y, depths[p])
    if (a.depths) {
        const double zd = a.depths[p];
        ac = particle_interpolator(g, 2, false, zd);
        af = particle_interpolator(g, 2, true, zd);
    }
    const double up = particle_interpolate(a.u, xf, yc, ac);
    const double vp = particle_interpolate(a.v, xc, yf, ac);
    const double wp = particle_interpolate(a.w, xc, yc, af);
    // x⁺ = x + ξ * up * Δt with the Cartesian metric 1 (exact)
    a.x[p] = particle_boundary(g.T[0], x + (up * a.dt), g.xL[0], g.xR[0], a.restitution);
    a.y[p] = particle_boundary(g.T[1], y + (vp * a.dt), g.xL[1], g.xR[1], a.restitution);
    if (!a.depths) a.z[p] = particle_boundary(g.T[2], z + (wp * a.dt), g.xL[2], g.xR[2], a.restitution);
}
#endif
