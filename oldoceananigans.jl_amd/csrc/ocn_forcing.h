// ocn_forcing.h -- the forcing term of the tendencies: `+ forcing(i, j, k, grid, clock, model_fields)`, the last term of
// u_velocity_tendency and its v / w / tracer siblings (Models/NonhydrostaticModels/nonhydrostatic_tendency_kernel_functions.jl:81-93).
//
// The forcings of src/Forcings/ that cross the C ABI:
//   Forcing(array)       F = array[i, j, k]                                  (forcing.jl:165-177, model_forcing.jl:29)
//   Relaxation           F = rate * mask(x, y, z) * (target(x, y, z, t) - φ)  (relaxation.jl:75-90)
//   a function           F = program(x, y, z, t, deps...), a recorded program  (continuous_forcing.jl:119-142; ocn_forcing_function.h)
//   MultipleForcings     F = F₁ + F₂ + ...                                    (multiple_forcings.jl)
// The built-in masks and targets of relaxation.jl (GaussianMask, PiecewiseLinearMask, LinearTarget) depend on ONE coordinate and not on
// time, so the host evaluates `rate * mask(node)` and `target(node)` at the forced field's own location over the haloed index range of
// that direction (a binder does it with the reference's own functions, `exp` included) and the device does only the `*` and `-` the
// reference does per cell:
//   F = (rate·mask)[ξ_m] * (target[ξ_t] - φ)
// with the zero target as `0.0 - φ` (Julia's `0 - φ`: φ = +0.0 gives +0.0, not -0.0) and the constant mask as the bare rate
// (`rate * 1` is the rate). A Relaxation whose mask or target is any other function is one function term (kind 3): this header's
// kernels never see it -- a field that has one is completed by forcing_function_kernel, which calls forcing_one for its other terms.
//
// Association order of a sum: N <= 4 terms are the explicit left-to-right sums of multiple_forcings.jl (F₁ + F₂ + F₃ + F₄); N > 4
// is its generated loop `total = zero(grid); total += Fₙ`, i.e. ((0.0 + F₁) + F₂) + ... The tendency is completed as
// G = G_rest + F; Flux-condition terms come after (compute_flux_bc_tendencies!).
//
// The per-field descriptors live in ONE device-resident table (ForcingTable, owned by the model, rewritten by
// ocn_model_set_forcing only): kernels receive its address, not a by-value copy of the descriptors.
#pragma once
#include "ocn_device.h"

#ifndef OCN_MAX_FORCING_TERMS
#define OCN_MAX_FORCING_TERMS 8        // (include/ocn_mi355x.h)
#endif
#define OCN_FORCING_KIND_ARRAY 1
#define OCN_FORCING_KIND_RELAXATION 2

struct ForcingTerm {
    int kind;
    int mask_dir, target_dir;        // -1: the constant below; 0 / 1 / 2: the table along x / y / z
    double rate_mask, target;
    const double *array;             // ARRAY: (Center, Center, Center) parent layout of the model's grid (borrowed)
    const double *mask_table;        // rate * mask(node), indexed [ξ - 1 + H_ξ] (library-owned copy)
    const double *target_table;      // target(node), same indexing
};

struct ForcingTable {
    int nterms[OCN_MAX_FIELDS];
    Range6 r[OCN_MAX_FIELDS];        // the range the tendency launch covers for the field (kernel_launching.jl:145-195)
    int s1[OCN_MAX_FIELDS];          // parent strides of the field (its location) ...
    long s2[OCN_MAX_FIELDS], off[OCN_MAX_FIELDS];
    int as1;                         // ... and of a (Center, Center, Center) array
    long as2, aoff;
    ForcingTerm t[OCN_MAX_FIELDS][OCN_MAX_FORCING_TERMS];
};

__device__ __forceinline__ int forcing_table_index(const DGrid &g, int dir, int i, int j, int k) {
    return dir == 0 ? i - 1 + g.Hx : (dir == 1 ? j - 1 + g.Hy : k - 1 + g.Hz);
}

__device__ __forceinline__ double forcing_one(const ForcingTable *__restrict__ tab, const ForcingTerm &T, const DGrid &g, int i, int j, int k,
                                              double phi) {
    if (T.kind == OCN_FORCING_KIND_ARRAY) return T.array[tab->aoff + i + (long)tab->as1 * j + tab->as2 * k];
    const double a = T.mask_dir < 0 ? T.rate_mask : T.mask_table[forcing_table_index(g, T.mask_dir, i, j, k)];
    const double b = T.target_dir < 0 ? T.target : T.target_table[forcing_table_index(g, T.target_dir, i, j, k)];
    return a * (b - phi);
}

// the forcing of field f at (i, j, k) -- φ is the field's own value there -- in the reference's association order
__device__ __forceinline__ double forcing_sum(const ForcingTable *__restrict__ tab, int f, const DGrid &g, int i, int j, int k, double phi) {
    const int n = tab->nterms[f];
    const ForcingTerm *T = tab->t[f];
    if (n > 4) {
        double total = 0.0;
#pragma unroll 1
        for (int q = 0; q < n; ++q) total += forcing_one(tab, T[q], g, i, j, k, phi);
        return total;
    }
    double s = forcing_one(tab, T[0], g, i, j, k, phi);
#pragma unroll 1
    for (int q = 1; q < n; ++q) s = s + forcing_one(tab, T[q], g, i, j, k, phi);
    return s;
}

struct ForcingLaunch {
    int n;                               // forced fields in this launch
    int f[OCN_MAX_FIELDS];               // their model field indices
    const double *U[OCN_MAX_FIELDS];     // φ (the prognostic field the tendency was evaluated from)
    double *G[OCN_MAX_FIELDS];           // the tendency being completed
};

// standalone pass: G[f] = G[f] + F over the range the tendency launch covered, every forced field in one launch
// (grid: x / y tiles of the largest range, z = levels x forced fields)
__global__ void __launch_bounds__(256) add_forcing_kernel(DGrid g, const ForcingTable *__restrict__ tab, ForcingLaunch L, int nk) {
    const int q = blockIdx.z / nk, kk = blockIdx.z - q * nk;
    const int f = L.f[q];
    const Range6 r = tab->r[f];
    const int i = r.i0 + blockIdx.x * blockDim.x + threadIdx.x, j = r.j0 + blockIdx.y * blockDim.y + threadIdx.y, k = r.k0 + kk;
    if (i > r.i1 || j > r.j1 || k > r.k1) return;
    const long o = tab->off[f] + i + (long)tab->s1[f] * j + tab->s2[f] * k;
    const double phi = L.U[q][o];
    L.G[q][o] = L.G[q][o] + forcing_sum(tab, f, g, i, j, k, phi);
}
