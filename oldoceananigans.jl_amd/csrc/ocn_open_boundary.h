// ocn_open_boundary.h -- OpenBoundaryCondition(value; scheme = PerturbationAdvection(inflow_timescale, outflow_timescale))
// (BoundaryConditions/perturbation_advection.jl) and enforce_open_boundary_mass_conservation!
// (Models/NonhydrostaticModels/boundary_mass_fluxes.jl) for the wall-normal velocities of a RectilinearGrid.
//
// Four kernels, every one launched over a LIST of boundary faces (at most six: west / east of u, south / north of v, bottom / top of w),
// 256 threads per block, one thread per face point, the blocks of one face contiguous in the launch:
//   open_boundary_carry_kernel    the boundary values follow the model's fields from one set of arrays into the other
//   open_boundary_step_kernel     step_left_boundary! / step_right_boundary! (:71-117) on every face of the list
//   open_boundary_flux_kernel     per-block partial sums of u Ax, v Ay, w Az (+ on left faces, - on right faces): launch A
//   open_boundary_correct_kernel  every block adds the partials in one fixed order, forms A⁻¹ ∮u dA and applies it to its face points
//                                 (- on left faces, + on right ones, :200-238): launch B
// No atomics and no host round trip; the order of every sum is fixed by the launch geometry, so two runs give the same bits.
// Arithmetic: the translation unit is compiled with -ffp-contract=off, the division is the IEEE one.
#pragma once
#include "ocn_device.h"
#include <cmath>

#define OB_THREADS 256

// PerturbationAdvection(inflow_timescale = 0, outflow_timescale = Inf) on one side (perturbation_advection.jl:4-7,57-63); on = false: the
// imposed form, scheme = nothing
struct OpenScheme { bool on = false; double tin = 0.0, tout = INFINITY; };

struct ObFace {
    double *p;                  // the field's parent array
    const double *from;         // open_boundary_carry_kernel only: the array whose boundary values p takes over
    long iB, iA;                // parent index of the boundary / boundary-adjacent point at the tangential point (1, 1)
    long sa, sb;                // parent strides of the two tangential directions (x before y before z)
    int Na, Nb;                 // their interior extents
    int dir;                    // normal direction: 0 x, 1 y, 2 z
    int right;                  // 0: west / south / bottom, 1: east / north / top
    int first_block;            // the face's first block in the launch
    double dX;                  // Δxᶠᶜᶜ / Δyᶜᶠᶜ / Δzᶜᶜᶠ at the boundary index
    double value;               // ū: the condition, or ...
    const double *arr;          // ... its dense (Na, Nb) array
    double tin, tout;           // inflow_timescale, outflow_timescale
};
struct ObFaces {
    int n, nblocks;
    ObFace f[6];
};

// the face of a block and the face point of a thread (-1: none)
__device__ __forceinline__ int ob_face_of_block(const ObFaces &S) {
    int q = 0;
    while (q + 1 < S.n && (int)blockIdx.x >= S.f[q + 1].first_block) ++q;
    return q;
}

// Julia's min / max of two Float64: a NaN operand gives NaN (fmin / fmax would drop it)
__device__ __forceinline__ double jl_min(double x, double y) { return (x != x || y != y) ? (x + y) : (y < x ? y : x); }
__device__ __forceinline__ double jl_max(double x, double y) { return (x != x || y != y) ? (x + y) : (y > x ? y : x); }

// dt: clock.last_stage_Δt, already 0 where it was Inf (:75-76, :99-100)
__global__ void __launch_bounds__(OB_THREADS) open_boundary_step_kernel(ObFaces S, double dt) {
    const ObFace &s = S.f[ob_face_of_block(S)];
    const long t = (long)((int)blockIdx.x - s.first_block) * OB_THREADS + threadIdx.x;
    if (t >= (long)s.Na * s.Nb) return;
    const long off = (t % s.Na) * s.sa + (t / s.Na) * s.sb;
    const double ubar = s.arr ? s.arr[t] : s.value;                 // ūⁿ⁺¹ = getbc(bc, l, m, grid, clock, model_fields)
    const double uB = s.p[s.iB + off];                              // uᵢⁿ
    const double uA = s.p[s.iA + off];                              // uᵢ₋₁ⁿ⁺¹
    const double c = dt / s.dX * ubar;                              // Δt / ΔX * ūⁿ⁺¹
    double unew;
    if (s.right) {
        const double U = jl_max(0.0, jl_min(1.0, c));               // :81
        const double tau = ubar >= 0 ? s.tout : s.tin;              // :84
        if (tau == 0) unew = ubar;                                  // :88 (the quotient would be NaN / Inf and is discarded)
        else {
            const double tt = dt / tau;                             // :85
            unew = (uB + U * uA + ubar * tt) / (1 + tt + U);        // :87
        }
    } else {
        const double U = jl_min(0.0, jl_max(-1.0, c));              // :105
        const double tau = ubar <= 0 ? s.tout : s.tin;              // :108
        if (tau == 0) unew = ubar;                                  // :112
        else {
            const double tt = dt / tau;                             // :109
            unew = (uB - U * uA + ubar * tt) / (1 + tt - U);        // :111
        }
    }
    s.p[s.iB + off] = unew;
}

// p[boundary] = from[boundary]: a substep that rode in the tendency launch wrote the interior of the fields into a second set of arrays
// (ocn_model_s::U2) and never writes a wall face, whose value -- the scheme's state -- is carried over here when the two sets swap
__global__ void __launch_bounds__(OB_THREADS) open_boundary_carry_kernel(ObFaces S) {
    const ObFace &s = S.f[ob_face_of_block(S)];
    const long t = (long)((int)blockIdx.x - s.first_block) * OB_THREADS + threadIdx.x;
    if (t >= (long)s.Na * s.Nb) return;
    const long at = s.iB + (t % s.Na) * s.sa + (t / s.Na) * s.sb;
    s.p[at] = s.from[at];
}

// sum of the block's values in a fixed order (a tree over the thread index), valid in thread 0
__device__ __forceinline__ double ob_block_sum(double x, double *lds) {
    lds[threadIdx.x] = x;
    __syncthreads();
    for (int w = OB_THREADS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) lds[threadIdx.x] += lds[threadIdx.x + w];
        __syncthreads();
    }
    return lds[0];
}

// launch A: partial[block] = ± Σ u A over the block's face points; A = Axᶠᶜᶜ = Δy Δzᶜ[k], Ayᶜᶠᶜ = Δx Δzᶜ[k] or Azᶜᶜᶠ = Δx Δy
__global__ void __launch_bounds__(OB_THREADS) open_boundary_flux_kernel(ObFaces S, DGrid g, double *partial) {
    __shared__ double lds[OB_THREADS];
    const ObFace &s = S.f[ob_face_of_block(S)];
    const long t = (long)((int)blockIdx.x - s.first_block) * OB_THREADS + threadIdx.x;
    double x = 0.0;
    if (t < (long)s.Na * s.Nb) {
        const int b = (int)(t / s.Na);
        const double area = s.dir == 2 ? g.az : (s.dir == 0 ? g.ax[b + g.Hz] : g.ay[b + g.Hz]);      // b = k - 1
        x = s.p[s.iB + (t % s.Na) * s.sa + b * s.sb] * area;
    }
    const double sum = ob_block_sum(x, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = s.right ? -sum : sum;
}

// launch B over the faces that carry a scheme: total = Σ partial (fixed order) + host_flux (the constant imposed faces, condition area,
// signed), correction = total / area; left faces -= correction, right faces += correction. total_out (may be null): where block 0 stores
// the total -- the diagnostic open_boundary_mass_inflow; with S.n == 0 that is all the launch does.
__global__ void __launch_bounds__(OB_THREADS) open_boundary_correct_kernel(ObFaces S, const double *partial, int npartial, double host_flux,
                                                                         double area, double *total_out) {
    __shared__ double lds[OB_THREADS];
    double x = 0.0;
    for (int q = threadIdx.x; q < npartial; q += OB_THREADS) x += partial[q];
    const double total = ob_block_sum(x, lds) + host_flux;
    if (total_out && blockIdx.x == 0 && threadIdx.x == 0) *total_out = total;
    if (S.n == 0) return;
    const ObFace &s = S.f[ob_face_of_block(S)];
    const long t = (long)((int)blockIdx.x - s.first_block) * OB_THREADS + threadIdx.x;
    if (t >= (long)s.Na * s.Nb) return;
    const double corr = total / area;                               // A⁻¹_∮udA = ∮udA / A (:230)
    const long at = s.iB + (t % s.Na) * s.sa + (t / s.Na) * s.sb;
    s.p[at] = s.right ? s.p[at] + corr : s.p[at] - corr;            // :200-214
}
