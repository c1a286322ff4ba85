// ocn_immersed.h -- grid-fitted immersed boundaries (ImmersedBoundaryGrid with GridFittedBottom / GridFittedBoundary): the two flag
// tables a grid carries, the kernel that builds them, the view the immersed instantiations of the tendency kernels read them through,
// and the masking kernel. gfx950 / wave64.
//
// The kernels of a time-step never evaluate inactive_node themselves: ocn_grid_set_immersed_boundary runs immersed_flags_kernel once over
// the whole parent extent of the cell mask (1 = immersed, halos filled by the caller) and everything else reads two tables, parent-shaped
// at (Center, Center, Center):
//
//   periphery, one byte per cell
//     bit 0      inactive_cell(i, j, k, ibg) = immersed_cell | inactive_cell(underlying grid)  (immersed_boundary_interface.jl:49,
//                Grids/inactive_node.jl:43-112)
//     bits 1..7  immersed_peripheral_node(i, j, k, ibg, ℓx, ℓy, ℓz) = peripheral_node(ibg) & !peripheral_node(underlying grid)
//                (immersed_boundary_interface.jl:53-54, inactive_node.jl:152-162) at fcc, cfc, ccf, ffc, fcf, cff, ccc: the seven locations
//                conditional_flux_* names (Advection/immersed_advective_fluxes.jl:20-59, TurbulenceClosures/immersed_diffusive_fluxes.jl:
//                27-44) and mask_immersed_field! tests (mask_immersed_field.jl:60-64)
//
//   orders, 16 bits per cell: per direction d (x, y, z) and side s (0: ᶠ, an interpolation to a Face; 1: ᶜ, to a Center) two bits at
//     shift 2 (2 d + s): the largest buffer b in {1, 2, 3} whose window holds no inactive node; 1 when none does (UpwindBiased{1} and
//     Centered{1} are not conditioned, immersed_advective_fluxes.jl:210). The window is the one inside_immersed_boundary lists
//     (immersed_advective_fluxes.jl:121-152): 2 b nodes for `:none` (symmetric) and for `:interior` (biased) alike -- N = 2b, or
//     N = 2b - 1 and rng = 1:N+1 -- at offsets -b .. b - 1 (ᶠ) or 1 - b .. b (ᶜ) along d. The node that is tested lies at the FLIPPED
//     location along d and at Center across it: `xside = side` is the only keyword the callers pass (:175-181), yside / zside stay at
//     their default :ᶠ, whose flip is c. So a window depends on the direction and the side only, and one entry serves
//     _symmetric_interpolate_* and _biased_interpolate_* of every field. Windows nest, so `order >= b` says the window of buffer b is free.
//
// The cascade is the reference's: _biased_interpolate falls WENO{3} -> WENO{2} -> UpwindBiased{1}, _symmetric_interpolate falls with it,
// WENO{3}'s advecting_velocity_scheme Centered(order = 4) -> Centered(order = 2) of WENO{2} and of UpwindBiased{1}
// (weno_reconstruction.jl:81-93, upwind_biased_reconstruction.jl:24-29,52-57), selected by the order entry instead of outside_*_halo:
// the reference defines the immersed methods for every ImmersedBoundaryGrid and inactive_node of such a grid already counts the cells
// outside a Bounded domain. At a wall both predicates read i >= b + 1 (ᶠ) / i >= b (ᶜ) and i <= N + 1 - b.
//
// A Flat direction has one cell and no halo: a shift along it is no shift (its Face is its Center), which the zero strides of the view
// express. The windows reach b cells from a Center-side index that itself runs from 0: an immersed grid needs a halo of buffer + 1
// (inflate_halo_size_one_dimension(req, old, _, ::IBG) = max(req + 1, old)), which ocn_grid_set_immersed_boundary checks.
#pragma once
#include "ocn_device.h"

enum { IMM_INACTIVE = 0, IMM_FCC = 1, IMM_CFC = 2, IMM_CCF = 3, IMM_FFC = 4, IMM_FCF = 5, IMM_CFF = 6, IMM_CCC = 7 };

// what the plain instantiations pass where the immersed ones pass an ImmView: no data, every test a compile-time `false`
struct NoImm {
    static constexpr bool on = false;
    __device__ __forceinline__ static double flux(int, int, int, int, double q) { return q; }      // no boundary: every flux is itself
};

// The two tables of a grid, addressed with the reference's 1-based (i, j, k). Kept out of DGrid -- that struct is a by-value argument of
// nearly every kernel -- and handed to the immersed instantiations only.
struct ImmView {
    static constexpr bool on = true;
    const unsigned char *periph;
    const unsigned short *orders;
    int sx, sy;                 // strides along x and y: 0 along a Flat direction
    long sz;
    long off;
    __device__ __forceinline__ long lin(int i, int j, int k) const { return off + (long)sx * i + (long)sy * j + sz * k; }
    __device__ __forceinline__ bool bit(int b, int i, int j, int k) const { return (periph[lin(i, j, k)] >> b) & 1; }
    // conditional_flux(i, j, k, ibg, ℓx, ℓy, ℓz, zero(ibg), q): ifelse, so q is evaluated either way
    __device__ __forceinline__ double flux(int b, int i, int j, int k, double q) const { return bit(b, i, j, k) ? 0.0 : q; }
    // the largest free buffer of the window along D on side CEN at the index the _interpolate function is called with
    template <int D, bool CEN> __device__ __forceinline__ int order(int i, int j, int k) const {
        return (orders[lin(i, j, k)] >> (2 * (2 * D + (CEN ? 1 : 0)))) & 3;
    }
};

// the location a momentum flux lives at: psi is a Face field along DS (the direction its advecting transport is interpolated along), the
// flux points along DB -- ccc when they coincide, else Face in both (immersed_advective_fluxes.jl:39-55)
template <int DS, int DB> __host__ __device__ constexpr int imm_momentum_flux_bit() {
    return DS == DB ? IMM_CCC : ((DS + DB == 1) ? IMM_FFC : ((DS + DB == 2) ? IMM_FCF : IMM_CFF));
}

// _symmetric_interpolate on an immersed grid: Centered(order = 4) where the window of buffer 3 is free, else Centered(order = 2); the
// arithmetic is symmetric_interp's
__device__ __forceinline__ double symmetric_interp_order(double q0, double q1, double q2, double q3, int order) {
    const double c4 = __builtin_fma(OCN_C4_1, q3, __builtin_fma(OCN_C4_2, q2, __builtin_fma(OCN_C4_3, q1, OCN_C4_4 * q0)));
    if (order >= 3) return c4;
    return __builtin_fma(OCN_C2_1, q2, OCN_C2_2 * q1);
}

// _biased_interpolate on an immersed grid: WENO{3}, WENO{2}, UpwindBiased{1} by the order entry (already capped by the direction's own
// scheme); the arithmetic is biased_interp's. s0..s5 = psi[f-3 .. f+2]
__device__ __forceinline__ double biased_interp_order(double s0, double s1, double s2, double s3, double s4, double s5, bool left, int order) {
    if (order >= 3) return weno5_biased<0>(s0, s1, s2, s3, s4, s5, left);
    if (order == 2) return weno3_biased(s1, s2, s3, s4, left);
    return left ? 1.0 * s2 : 1.0 * s3;
}

// ---------------------------------------------------------------------------------------------------------------------
// the flag tables from the cell mask: one thread per cell of the parent extent
// ---------------------------------------------------------------------------------------------------------------------
struct ImmGeometry {
    int N[3], H[3], T[3];       // size, halo, topology code per direction
};

__global__ void __launch_bounds__(256) immersed_flags_kernel(ImmGeometry G, const unsigned char *__restrict__ cell, unsigned char *__restrict__ periph,
                                                             unsigned short *__restrict__ orders) {
    const int P0 = G.N[0] + 2 * G.H[0], P1 = G.N[1] + 2 * G.H[1], P2 = G.N[2] + 2 * G.H[2];
    const int p0 = blockIdx.x * blockDim.x + threadIdx.x, p1 = blockIdx.y * blockDim.y + threadIdx.y, p2 = blockIdx.z;
    if (p0 >= P0 || p1 >= P1 || p2 >= P2) return;
    const int I[3] = {p0 + 1 - G.H[0], p1 + 1 - G.H[1], p2 + 1 - G.H[2]};
    const int P[3] = {P0, P1, P2};
    // inactive_cell of the underlying grid (inactive_node.jl:43-112): beyond a wall. A Flat direction ignores its index.
    auto outside = [&](const int idx[3]) {
        bool out = false;
#pragma unroll
        for (int d = 0; d < 3; ++d) out = out || (wall_lo(G.T[d]) && idx[d] < 1) || (wall_hi(G.T[d]) && idx[d] > G.N[d]);
        return out;
    };
    // inactive_cell of the immersed grid (immersed_boundary_interface.jl:49). An index beyond the parent extent of a direction without a
    // wall there has no mask entry: not immersed -- only entries whose window leaves the halo see it, and none of those is read (header)
    auto inactive = [&](const int idx[3], bool underlying) {
        if (outside(idx)) return true;
        if (underlying) return false;
        long at = 0, stride = 1;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            if (G.T[d] != OCN_FLAT) {
                const int p = idx[d] - 1 + G.H[d];
                if (p < 0 || p >= P[d]) return false;
                at += stride * p;
            }
            stride *= P[d];
        }
        return cell[at] != 0;
    };
    auto shifted = [&](const int idx[3], int d, int n, int out[3]) {
#pragma unroll
        for (int q = 0; q < 3; ++q) out[q] = idx[q];
        if (G.T[d] != OCN_FLAT) out[d] += n;
    };
    // peripheral_node (inactive_node.jl:152-162) at a location given by its Face directions `faces` (bit d: Face along d): the `|` of
    // inactive_cell over the cells around the node
    auto peripheral = [&](int faces, bool underlying) {
        bool any = false;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            if (c & ~faces) continue;
            int idx[3] = {I[0], I[1], I[2]};
#pragma unroll
            for (int d = 0; d < 3; ++d)
                if (((c >> d) & 1) && G.T[d] != OCN_FLAT) idx[d] -= 1;
            any = any || inactive(idx, underlying);
        }
        return any;
    };
    const int faces_of[8] = {0, 1, 2, 4, 3, 5, 6, 0};          // bit -> Face directions: fcc, cfc, ccf, ffc, fcf, cff, ccc
    unsigned char byte = inactive(I, false) ? 1 : 0;
#pragma unroll
    for (int b = 1; b < 8; ++b)
        if (peripheral(faces_of[b], false) && !peripheral(faces_of[b], true)) byte |= (unsigned char)(1 << b);
    unsigned short word = 0;
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            int best = 1;
            if (G.T[d] == OCN_FLAT) best = 3;
            else
#pragma unroll
                for (int b = 3; b >= 2; --b) {
                    bool free_ = true;
#pragma unroll
                    for (int c = (side ? 1 - b : -b); c <= (side ? b : b - 1); ++c) {
                        int a[3], m[3];
                        shifted(I, d, c, a);
                        shifted(I, d, c - 1, m);
                        // ᶠ: inactive_node at ccc is inactive_cell; ᶜ: at the Face along d it is inactive_cell & inactive_cell one below
                        const bool node = side ? (inactive(a, false) && inactive(m, false)) : inactive(a, false);
                        free_ = free_ && !node;
                    }
                    if (free_) { best = b; break; }
                }
            word |= (unsigned short)(best << (2 * (2 * d + side)));
        }
    const long at = p0 + (long)P0 * (p1 + (long)P1 * p2);
    periph[at] = byte;
    orders[at] = word;
}

// ---------------------------------------------------------------------------------------------------------------------
// mask_immersed_field! (mask_immersed_field.jl:53-64) of up to OCN_MAX_FIELDS fields in one launch over :xyz -- all tracers, or all three
// velocities: field = masked ? value : field at immersed_peripheral_node of the field's own location
// ---------------------------------------------------------------------------------------------------------------------
struct ImmMaskList {
    int n;
    FView f[OCN_MAX_FIELDS];
    int bit[OCN_MAX_FIELDS];
};

__global__ void __launch_bounds__(256) mask_immersed_kernel(ImmView im, ImmMaskList L, double value, int Nx, int Ny, int Nz) {
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x;
    const int j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    const int q = blockIdx.z / Nz, k = 1 + blockIdx.z % Nz;
    if (i > Nx || j > Ny || q >= L.n) return;
    const unsigned char byte = im.periph[im.lin(i, j, k)];
#pragma unroll
    for (int f = 0; f < OCN_MAX_FIELDS; ++f)                 // (a constant trip count: the argument arrays are indexed statically)
        if (f == q && ((byte >> L.bit[f]) & 1)) L.f[f].at(i, j, k) = value;
}
