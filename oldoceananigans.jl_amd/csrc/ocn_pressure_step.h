// ocn_pressure_step.h -- the kernels on either side of the pressure solve and their host launchers: the source term of the pressure
// equation, the pressure correction, the copies between the solvers' dense real arrays and the haloed pressure field
// (src/Models/NonhydrostaticModels/{solve_for_pressure,pressure_correction}.jl). Included by ocn_api.hip ahead of the solvers.
//
// ONE implementation of each expression, whatever the layout:
//   * source_from_faces   divᶜᶜᶜ(u*) [x Δzᶜ] from the six face values of a cell -- every source kernel forms its value here;
//   * correct_velocities  u -= ∂x p, v -= ∂y p, w -= ∂z p, p / Δt⁺ -- every correction kernel corrects its cell here;
//   * dense_neighbours    (p, p[i-1], p[j-1], p[k-1]) of a cell in a dense x-fastest solution: the wrap in x or the received west column,
//                         the wrap in y, the wrap or the no-flux copy in z.
// The kernels differ in where the operands come from (haloed fields, wrapped interior indices, received columns, LDS tiles) and where the
// results go. Same operations on the same operands in the same order on every path (the build has -ffp-contract=off): the same bits.
#pragma once
#include "ocn_kernels.h"
#include "ocn_line_fft.h"

// ---------------------------------------------------------------------------------------------------------------------
// the source term: divᶜᶜᶜ(u*) [x Δzᶜ for the Fourier-tridiagonal solver] (solve_for_pressure.jl:12-84, Operators/divergence_operators.jl:16-19)
// ---------------------------------------------------------------------------------------------------------------------
// from the six face values of the cell at level kk = k - 1 + Hz: (u0, up) = u[i], u[i + 1], likewise v along y and w along z
// PLAIN: a layout that exists on grids without Flat directions and for the unweighted source only (the partitioned solvers' own kernels):
// no test of either
template <bool PLAIN = false>
__device__ __forceinline__ double source_from_faces(const DGrid &g, int kk, double u0, double up, double v0, double vp, double w0, double wp,
                                                    bool weight_by_dz = false) {
    const double ax = g.ax[kk], ay = g.ay[kk], az = g.az;
    // δ along a Flat direction is zero(FT) (Operators/difference_operators.jl:30-49)
    double dx = !PLAIN && g.tx == OCN_FLAT ? 0.0 : ax * up - ax * u0;      // δxᶜᶜᶜ(Ax_qᶠᶜᶜ, u)
    double dy = !PLAIN && g.ty == OCN_FLAT ? 0.0 : ay * vp - ay * v0;
    double dz = !PLAIN && g.tz == OCN_FLAT ? 0.0 : az * wp - az * w0;
    double div = g.vinv_c[kk] * ((dx + dy) + dz);                 // divᶜᶜᶜ, Operators/divergence_operators.jl:16-19
    return !PLAIN && weight_by_dz ? (1.0 * g.dzc[kk]) * div : 1.0 * div;
}
// ... with the faces read from the haloed velocities
// wrap: bit 0 / 1 / 2 = the upper x / y / z neighbour of the last cell is read at its wrapped interior index instead of the halo;
// ue (x-slab ranks): u[Nx + 1, j, k] is read from this dense (Ny, Nz) buffer -- the east neighbour's first column, just received
template <bool PLAIN = false>
__device__ __forceinline__ double source_value(const DGrid &g, const FView &u, const FView &v, const FView &w, int i, int j, int k,
                                               bool weight_by_dz, int wrap, const double *ue = nullptr) {
    const int ip = ((wrap & 1) && i == g.Nx) ? 1 : i + 1, jp = ((wrap & 2) && j == g.Ny) ? 1 : j + 1, kp = ((wrap & 4) && k == g.Nz) ? 1 : k + 1;
    const double up = (ue && i == g.Nx) ? ue[(long)(j - 1) + (long)g.Ny * (k - 1)] : u.at(ip, j, k);
    // (a Flat direction has no upper neighbour to read)
    const bool fx = !PLAIN && g.tx == OCN_FLAT, fy = !PLAIN && g.ty == OCN_FLAT, fz = !PLAIN && g.tz == OCN_FLAT;
    return source_from_faces<PLAIN>(g, k - 1 + g.Hz, fx ? 0.0 : u.at(i, j, k), fx ? 0.0 : up, fy ? 0.0 : v.at(i, j, k), fy ? 0.0 : v.at(i, jp, k),
                                    fz ? 0.0 : w.at(i, j, k), fz ? 0.0 : w.at(i, j, kp), weight_by_dz);
}

template <bool REAL_OUT>
// rhs element (i, j, k) is stored at (i-1) + sj*(j-1) + sk*(k-1); `pad` (real output only): the row has one extra, zero,
// element after i = Nx (odd local Nx on the distributed solver's paired-column layout)
// wrap (Periodic directions only): the upper neighbours are read at their wrapped INTERIOR index instead of the halo, so the
// velocity halo fill that precedes the solve in the reference can be left to the next update_state! (same values by construction)
__global__ void __launch_bounds__(256) source_term_kernel(DGrid g, FView u, FView v, FView w, void *rhs, bool weight_by_dz,
                                                          long sj, long sk, bool pad, int wrap = 0, const double *ue = nullptr) {
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x;
    const int j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    const int k = 1 + blockIdx.z;
    if (i > g.Nx || j > g.Ny || k > g.Nz) return;
    const double val = source_value(g, u, v, w, i, j, k, weight_by_dz, wrap, ue);
    const long q = (long)(i - 1) + sj * (j - 1) + sk * (k - 1);
    if (REAL_OUT) {                                         // real-transform paths (rhs is real by construction)
        ((double *)rhs)[q] = val;
        if (pad && i == g.Nx) ((double *)rhs)[q + 1] = 0.0;
    } else ((double2 *)rhs)[q] = make_double2(val, 0.0);    // the reference's complex storage
}

// Stage 1 of an RK3 step on a triply periodic grid: rk3_substep_kernel (no ζ term) and source_term_kernel<true> (wrap = 7) in one pass.
// The tracers are advanced in place. u*, v*, w* = U + Δt γ G are formed for the cell and for its three upper neighbours (at the wrapped
// interior index: G is zero in the halo) but NOT stored: a neighbour's thread may run before or after this one, so an in-place store
// would let it read u* where it expects U. pressure_correction_periodic_kernel<., true> forms the same u* again -- the same expression
// on the same operands, the same bits -- and corrects it, so the velocities are still read once and written once per stage.
__global__ void __launch_bounds__(256) substep_source_kernel(DGrid g, SubstepArgs a, double dt, double gamma, double *rhs, bool weight_by_dz) {
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x;
    const int j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    const int k = 1 + blockIdx.z;
    if (i > g.Nx || j > g.Ny || k > g.Nz) return;
    for (int f = 3; f < a.n; ++f) {
        const long q = a.view[f].lin(i, j, k);
        double Uv = a.U[f][q];
        Uv += dt * gamma * a.Gn[f][q];
        a.U[f][q] = Uv;
    }
    const int ip = i == g.Nx ? 1 : i + 1, jp = j == g.Ny ? 1 : j + 1, kp = k == g.Nz ? 1 : k + 1;
    const long qu = a.view[0].lin(i, j, k), qup = a.view[0].lin(ip, j, k);
    const long qv = a.view[1].lin(i, j, k), qvp = a.view[1].lin(i, jp, k);
    const long qw = a.view[2].lin(i, j, k), qwp = a.view[2].lin(i, j, kp);
    const double u0 = a.U[0][qu] + dt * gamma * a.Gn[0][qu], up = a.U[0][qup] + dt * gamma * a.Gn[0][qup];
    const double v0 = a.U[1][qv] + dt * gamma * a.Gn[1][qv], vp = a.U[1][qvp] + dt * gamma * a.Gn[1][qvp];
    const double w0 = a.U[2][qw] + dt * gamma * a.Gn[2][qw], wp = a.U[2][qwp] + dt * gamma * a.Gn[2][qwp];
    rhs[(long)(i - 1) + (long)g.Nx * ((j - 1) + (long)g.Ny * (k - 1))] = source_from_faces(g, k - 1 + g.Hz, u0, up, v0, vp, w0, wp, weight_by_dz);
}

// compute_source_term! into a dense real array stored z-fastest, r[(k-1) + Nz*((i-1) + Nx*(j-1))] (the layout a unit-stride R2C along z
// wants): the divergence is evaluated with threads along x (coalesced reads), transposed through an LDS tile and written with threads
// along z. z Periodic (unweighted). wrap = 0: from the halos; wrap = 6 with ue (the partitioned model's fused step): no halo is read -- y / z
// neighbours at wrapped interior indices, u[Nx+1, j, k] = ue[j-1 + Ny (k-1)], the column received by the one-column exchange.
__global__ void __launch_bounds__(256) source_term_zfast_kernel(DGrid g, FView u, FView v, FView w, int wrap, const double *ue, double *r) {
    __shared__ double tile[32][33];
    const int i0 = 1 + blockIdx.x * 32, k0 = 1 + blockIdx.y * 32, j = 1 + blockIdx.z;
    const int tx = threadIdx.x, ty = threadIdx.y;          // block (32, 8)
    for (int kk = ty; kk < 32; kk += 8) {
        const int i = i0 + tx, k = k0 + kk;
        if (i <= g.Nx && k <= g.Nz) tile[kk][tx] = source_value<true>(g, u, v, w, i, j, k, false, wrap, ue);
    }
    __syncthreads();
    for (int ii = ty; ii < 32; ii += 8) {
        const int k = k0 + tx, i = i0 + ii;
        if (i <= g.Nx && k <= g.Nz) r[(long)(k - 1) + (long)g.Nz * ((i - 1) + (long)g.Nx * (j - 1))] = tile[tx][ii];
    }
}

// source_term_kernel<true> (wrap = 6, ue) + paired_zline_r2c_kernel in ONE pass: the divergences of a column pair go straight into the LDS line
// buffer of the z transform instead of through the dense real array (a write and a read of N^3 doubles less per solve: 0.105 + 0.075 -> 0.153 ms
// at 256^3; unrolling the level loop changes nothing). Same expressions on
// the same operands as the two kernels => the same bits. Pair c covers the columns (2c, 2c + 1) of the (x, y) plane, x fastest (Nx even).
template <int ZL>
__global__ void __launch_bounds__(256) source_paired_zline_r2c_kernel(DGrid g, FView u, FView v, FView w, const double *ue, double2 *spec, const double2 *tw,
                                                                      long C, int N, int logn) {
    extern __shared__ double2 zbuf[];                 // [N][ZL]
    const int il = threadIdx.x % ZL, kq = threadIdx.x / ZL, KQ = 256 / ZL;
    const long c = (long)blockIdx.x * ZL + il;
    const bool live = c < C;
    const int hx = g.Nx >> 1;
    const int j = live ? (int)(c / hx) + 1 : 1, i0 = live ? 2 * (int)(c % hx) + 1 : 1;
    const int jp = j == g.Ny ? 1 : j + 1;
    for (int kk = kq; kk < N; kk += KQ) {
        const int k = kk + 1, kt = k - 1 + g.Hz, kp = k == g.Nz ? 1 : k + 1;
        const double u0 = u.at(i0, j, k), u1 = u.at(i0 + 1, j, k);
        const double u2 = (i0 + 1 == g.Nx && ue) ? ue[(long)(j - 1) + (long)g.Ny * (k - 1)] : u.at(i0 + 2, j, k);
        const double v0 = v.at(i0, j, k), v1 = v.at(i0 + 1, j, k), v0p = v.at(i0, jp, k), v1p = v.at(i0 + 1, jp, k);
        const double w0 = w.at(i0, j, k), w1 = w.at(i0 + 1, j, k), w0p = w.at(i0, j, kp), w1p = w.at(i0 + 1, j, kp);
        const double d0 = source_from_faces<true>(g, kt, u0, u1, v0, v0p, w0, w0p), d1 = source_from_faces<true>(g, kt, u1, u2, v1, v1p, w1, w1p);
        zbuf[kk * ZL + il] = live ? make_double2(d0, d1) : make_double2(0.0, 0.0);
    }
    __syncthreads();
    lds_fft_forward(InterleavedLines<ZL>{zbuf, il, kq}, tw, N, logn);
    if (!live) return;
    paired_zline_separate<ZL>(zbuf, spec, c, C, N, logn, il, kq);
}

// ---------------------------------------------------------------------------------------------------------------------
// the correction: _make_pressure_correction! and `pNHS ./= Δt⁺` (pressure_correction.jl:31-50)
// ---------------------------------------------------------------------------------------------------------------------
struct PressureStencil { double pc, pim, pjm, pkm; };      // p Δt at (i, j, k), (i-1, j, k), (i, j-1, k), (i, j, k-1)

// u -= ∂xᶠᶜᶜ p, v -= ∂yᶜᶠᶜ p, w -= ∂zᶜᶜᶠ p (∂ = δ * Δ⁻¹) on the cell's three velocities, wherever the caller holds them (a reference into a
// field: read, corrected and stored here; a register: the caller stores it), and p / Δt⁺ -> *pstore unless that is NULL. Returns p / Δt⁺.
// PLAIN: the grid has no Flat direction (the dense-solution paths); otherwise δ along a Flat direction is zero and its neighbour was not read
template <bool PLAIN>
__device__ __forceinline__ double correct_velocities(const DGrid &g, int k, double &un, double &vn, double &wn, const PressureStencil &s,
                                                     double *pstore, double divisor) {
    un -= (!PLAIN && g.tx == OCN_FLAT ? 0.0 : s.pc - s.pim) * g.rdx;            // ∂xᶠᶜᶜ = δx * Δx⁻¹
    vn -= (!PLAIN && g.ty == OCN_FLAT ? 0.0 : s.pc - s.pjm) * g.rdy;
    wn -= (!PLAIN && g.tz == OCN_FLAT ? 0.0 : s.pc - s.pkm) * g.rdzf[k - 1 + g.Hz];
    const double ps = s.pc / divisor;
    if (pstore) *pstore = ps;
    return ps;
}

// the four values from a dense x-fastest real array that holds cell (i, j, k) at (i-1) + sj (j-1) + sk (k-1) -- (Nx, Nx Ny) for the
// single-GPU split solver and the x-fastest substructured solve, (Nxe Nz, Nxe) for the transposing solvers' paired-column layout.
// x: p[0, j, k] = pw[j-1 + Ny (k-1)] (a partitioned slab: the west neighbour's last column, received) or, without pw, the periodic wrap;
// y Periodic: wrapped; z Periodic: wrapped, zbounded: p[0] = p[1] (the no-flux halo of a Bounded z: the bottom face keeps its w)
__device__ __forceinline__ PressureStencil dense_neighbours(const DGrid &g, const double *pd, long sj, long sk, const double *pw, bool zbounded,
                                                            int i, int j, int k) {
    const long q = (long)(i - 1) + sj * (j - 1) + sk * (k - 1);
    PressureStencil s;
    s.pc = pd[q];
    s.pim = (pw && i == 1) ? pw[(long)(j - 1) + (long)g.Ny * (k - 1)] : pd[i == 1 ? q + (g.Nx - 1) : q - 1];
    s.pjm = pd[j == 1 ? q + sj * (g.Ny - 1) : q - sj];
    s.pkm = k == 1 ? (zbounded ? s.pc : pd[q + sk * (g.Nz - 1)]) : pd[q - sk];
    return s;
}

// from the haloed pressure field on a range of cells
// pdiv != nullptr: also `pNHS ./= Δt⁺`, written to a SECOND haloed array (neighbouring threads still read p) that the caller swaps in
__global__ void __launch_bounds__(256) pressure_correction_kernel(DGrid g, FView u, FView v, FView w, FView p, Range6 r,
                                                                  double *pdiv = nullptr, double divisor = 1.0) {
    const int i = r.i0 + blockIdx.x * blockDim.x + threadIdx.x;
    const int j = r.j0 + blockIdx.y * blockDim.y + threadIdx.y;
    const int k = r.k0 + blockIdx.z;
    if (i > r.i1 || j > r.j1 || k > r.k1) return;
    PressureStencil s;
    s.pc = p.at(i, j, k);
    s.pim = g.tx == OCN_FLAT ? 0.0 : p.at(i - 1, j, k);
    s.pjm = g.ty == OCN_FLAT ? 0.0 : p.at(i, j - 1, k);
    s.pkm = g.tz == OCN_FLAT ? 0.0 : p.at(i, j, k - 1);
    correct_velocities<false>(g, k, u.at(i, j, k), v.at(i, j, k), w.at(i, j, k), s, pdiv ? pdiv + p.lin(i, j, k) : nullptr, divisor);
}

// from the DENSE real array the inverse transform leaves, cell (i, j, k) of the columns the two kernels below hand out: no strided Z2D into
// the field, no halo fill of p, no divide pass. The haloed pressure field receives p / Δt⁺ when store_p.
__device__ __forceinline__ void dense_correction_cell(const DGrid &g, FView &u, FView &v, FView &w, const double *pd, const double *pw, FView &p,
                                                      double divisor, long sj, long sk, bool zbounded, bool store_p, int i, int j, int k) {
    const PressureStencil s = dense_neighbours(g, pd, sj, sk, pw, zbounded, i, j, k);
    correct_velocities<true>(g, k, u.at(i, j, k), v.at(i, j, k), w.at(i, j, k), s, store_p ? &p.at(i, j, k) : nullptr, divisor);
}
// the columns ia .. ib: the whole grid of a single-GPU model (pw = nullptr) or a range of a partitioned slab
__global__ void __launch_bounds__(256) pressure_correction_dense_slab_kernel(DGrid g, FView u, FView v, FView w, const double *pd, const double *pw,
                                                                             FView p, double divisor, int ia, int ib, long sj, long sk, bool zbounded,
                                                                             bool store_p) {
    const int i = ia + blockIdx.x * blockDim.x + threadIdx.x;
    const int j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    const int k = 1 + blockIdx.z;
    if (i > ib || j > g.Ny || k > g.Nz) return;
    dense_correction_cell(g, u, v, w, pd, pw, p, divisor, sj, sk, zbounded, store_p, i, j, k);
}
// ... and the two Hx-wide boundary strips of a slab (columns 1 .. H and Nx - H + 1 .. Nx) in one launch, threads along (column, y)
__global__ void __launch_bounds__(256) pressure_correction_dense_strips_kernel(DGrid g, FView u, FView v, FView w, const double *pd, const double *pw,
                                                                               FView p, double divisor, int H, long sj, long sk, bool zbounded, bool store_p) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x, j = 1 + blockIdx.y * blockDim.y + threadIdx.y, k = 1 + blockIdx.z;
    if (c >= 2 * H || j > g.Ny || k > g.Nz) return;
    dense_correction_cell(g, u, v, w, pd, pw, p, divisor, sj, sk, zbounded, store_p, c < H ? 1 + c : g.Nx - 2 * H + 1 + c, j, k);
}

// the dense correction on a triply periodic grid, with the passes that surround it folded in.
// SUBSTEP (RK3 stage 1 after substep_source_kernel): u, v, w still hold U; the thread forms u* = U + Δt γ G first, as rk3_substep_kernel does.
// FOLD: every halo cell of a periodic direction is a copy of an interior cell, and after this kernel u, v, w (and p / Δt⁺ when stored) are
// final until the next tendency evaluation, as the tracers `tr` already are. The thread of interior cell (i, j, k) therefore also writes its
// values to the periodic images of the cell -- per direction the offsets {0}, +N if the index <= H, -N if the index > N - H (both when
// N < 2H), every combination but (0, 0, 0) -- which is what fill_periodic_xyz_kernel would copy there. Only halo cells are written and
// none is read, so the threads do not depend on each other. All parents have the same shape (no Face field has an extra point).
template <bool FOLD, bool SUBSTEP>
__global__ void __launch_bounds__(256) pressure_correction_periodic_kernel(DGrid g, FView u, FView v, FView w, const double *pd, FView p,
                                                                           double divisor, bool store_p, FieldList tr, const double *Gu,
                                                                           const double *Gv, const double *Gw, double dt, double gamma) {
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x;
    const int j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    const int k = 1 + blockIdx.z;
    if (i > g.Nx || j > g.Ny || k > g.Nz) return;
    const PressureStencil s = dense_neighbours(g, pd, g.Nx, (long)g.Nx * g.Ny, nullptr, false, i, j, k);
    const long qu = u.lin(i, j, k), qv = v.lin(i, j, k), qw = w.lin(i, j, k), qc = p.lin(i, j, k);
    double un = u.p[qu], vn = v.p[qv], wn = w.p[qw];
    if (SUBSTEP) {
        un += dt * gamma * Gu[qu];
        vn += dt * gamma * Gv[qv];
        wn += dt * gamma * Gw[qw];
    }
    const double ps = correct_velocities<true>(g, k, un, vn, wn, s, store_p ? p.p + qc : nullptr, divisor);
    u.p[qu] = un;
    v.p[qv] = vn;
    w.p[qw] = wn;
    if (!FOLD) return;
    const bool lo[3] = {i <= g.Hx, j <= g.Hy, k <= g.Hz}, hi[3] = {i > g.Nx - g.Hx, j > g.Ny - g.Hy, k > g.Nz - g.Hz};
    if (!(lo[0] || hi[0] || lo[1] || hi[1] || lo[2] || hi[2])) return;
    for (int c = 0; c < 3; ++c) {                   // 0: the cell itself, 1: its image at +N, 2: at -N
        if ((c == 1 && !lo[2]) || (c == 2 && !hi[2])) continue;
        const int dk = c == 0 ? 0 : (c == 1 ? g.Nz : -g.Nz);
        for (int b = 0; b < 3; ++b) {
            if ((b == 1 && !lo[1]) || (b == 2 && !hi[1])) continue;
            const int dj = b == 0 ? 0 : (b == 1 ? g.Ny : -g.Ny);
            for (int a = 0; a < 3; ++a) {
                if ((a == 1 && !lo[0]) || (a == 2 && !hi[0]) || (a == 0 && b == 0 && c == 0)) continue;
                const int di = a == 0 ? 0 : (a == 1 ? g.Nx : -g.Nx);
                u.p[qu + di + (long)u.s1 * dj + u.s2 * dk] = un;
                v.p[qv + di + (long)v.s1 * dj + v.s2 * dk] = vn;
                w.p[qw + di + (long)w.s1 * dj + w.s2 * dk] = wn;
                const long d = di + (long)p.s1 * dj + p.s2 * dk;
                if (store_p) p.p[qc + d] = ps;
                for (int t = 0; t < tr.n; ++t) tr.p[t][qc + d] = tr.p[t][qc];
            }
        }
    }
}

// The x-slab pressure step without the passes between its stages (z Periodic, substructured x solve, z-fastest layout):
//   * the source term reads its periodic neighbours at wrapped interior indices and u[Nx+1] from the receive buffer of the one-column
//     exchange: no local fill, no unpack before it;
//   * the pressure correction reads the z-fastest real solution the inverse transform leaves (tiles transposed through LDS, the row
//     j - 1 kept from the previous iteration of a short march along y) and p[0] from the receive buffer: no copy_real pass, no haloed
//     copy of p dt, no fill / unpack of it;
//   * the pack of the early exchange reads wrapped interior rows / levels: no local fill of the strips before it.
// From the z-fastest dense solution pd[(k-1) + Nz ((i-1) + Nx (j-1))] = p Δt, columns ia .. ib. A block owns a 32 (x) x 32 (z) tile and
// marches over JB rows of y: the tile of row j (with one more column on its low x side and one more level on its low z side) is transposed
// through LDS, the tile of row j - 1 is the previous iteration's. x: p[0, j, k] = pw[k-1 + Nz (j-1)] (the west neighbour's last column,
// received); y, z Periodic: wrapped.
#define OCN_ZC_JB 8
__global__ void __launch_bounds__(256) pressure_correction_zfast_kernel(DGrid g, FView u, FView v, FView w, const double *pd, const double *pw,
                                                                        FView p, double divisor, int ia, int ib) {
    __shared__ double T[2][33][33];                   // [buffer][x: i0-1 .. i0+31][z: k0-1 .. k0+31]; odd pitch: no bank conflicts either way
    const int i0 = ia + blockIdx.x * 32, k0 = 1 + blockIdx.y * 32, jfirst = 1 + blockIdx.z * OCN_ZC_JB;
    const int tx = threadIdx.x, ty = threadIdx.y;     // block (32, 8)
    const long sNz = g.Nz, sNx = g.Nx;
    const int ni = min(min(ib, g.Nx), i0 + 31) - (i0 - 1) + 1;      // columns i0 - 1 .. min(ib, Nx, i0 + 31) of the tile
    auto load = [&](int buf, int j) {                 // threads along z (the fast index of pd)
        const int jw = j < 1 ? g.Ny : j;
        for (int ii = ty; ii < ni; ii += 8) {
            const int i = i0 - 1 + ii;
            for (int kk = tx; kk < 33; kk += 32) {
                int k = k0 - 1 + kk;
                if (k > g.Nz) continue;
                if (k < 1) k = g.Nz;
                T[buf][ii][kk] = i < 1 ? pw[(long)(k - 1) + sNz * (jw - 1)] : pd[(long)(k - 1) + sNz * ((i - 1) + sNx * (jw - 1))];
            }
        }
    };
    load(0, jfirst - 1);
    int cur = 1;
    for (int j = jfirst; j < jfirst + OCN_ZC_JB && j <= g.Ny; ++j, cur ^= 1) {
        __syncthreads();                              // the previous iteration's readers of T[cur] are done
        load(cur, j);
        __syncthreads();
        const int i = i0 + tx;
        if (i <= ib && i <= g.Nx) {
            // the three fields may alias as far as the compiler knows: load the four levels of u, v, w first, then store
            double uo[4], vo[4], wo[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k = min(k0 + ty + 8 * q, g.Nz);
                uo[q] = u.at(i, j, k); vo[q] = v.at(i, j, k); wo[q] = w.at(i, j, k);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int kk = ty + 8 * q, k = k0 + kk;
                if (k > g.Nz) continue;
                const PressureStencil s{T[cur][tx + 1][kk + 1], T[cur][tx][kk + 1], T[cur ^ 1][tx + 1][kk + 1], T[cur][tx + 1][kk]};
                correct_velocities<true>(g, k, uo[q], vo[q], wo[q], s, &p.at(i, j, k), divisor);
                u.at(i, j, k) = uo[q];
                v.at(i, j, k) = vo[q];
                w.at(i, j, k) = wo[q];
            }
        }
    }
}

// the same for the two Hx-wide boundary strips (columns 1 .. H and Nx - H + 1 .. Nx) in one launch: a tile kernel would leave 29 of 32
// lanes idle, so here a thread owns one cell and reads its four pressure values from the z-fastest array directly -- threads along
// (column, y) like pressure_correction_kernel on a strip range (8 columns per block: ceil(2 H / 8) blocks along x); the lines of pd are
// shared by 16 consecutive levels (L2)
__global__ void __launch_bounds__(256) pressure_correction_zfast_strips_kernel(DGrid g, FView u, FView v, FView w, const double *pd, const double *pw,
                                                                               FView p, double divisor, int H) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x, j = 1 + blockIdx.y * blockDim.y + threadIdx.y, k = 1 + blockIdx.z;
    if (c >= 2 * H || j > g.Ny || k > g.Nz) return;
    const int i = c < H ? 1 + c : g.Nx - 2 * H + 1 + c;
    const long sNz = g.Nz, sNx = g.Nx;
    const int jm = j == 1 ? g.Ny : j - 1, km = k == 1 ? g.Nz : k - 1;
    PressureStencil s;
    s.pc = pd[(long)(k - 1) + sNz * ((i - 1) + sNx * (j - 1))];
    s.pim = i == 1 ? pw[(long)(k - 1) + sNz * (j - 1)] : pd[(long)(k - 1) + sNz * ((i - 2) + sNx * (j - 1))];
    s.pjm = pd[(long)(k - 1) + sNz * ((i - 1) + sNx * (jm - 1))];
    s.pkm = pd[(long)(km - 1) + sNz * ((i - 1) + sNx * (j - 1))];
    correct_velocities<true>(g, k, u.at(i, j, k), v.at(i, j, k), w.at(i, j, k), s, &p.at(i, j, k), divisor);
}

__global__ void __launch_bounds__(256) divide_interior_kernel(DGrid g, FView p, double divisor) {
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x;
    const int j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    const int k = 1 + blockIdx.z;
    if (i > g.Nx || j > g.Ny || k > g.Nz) return;
    p.at(i, j, k) /= divisor;
}

// ---------------------------------------------------------------------------------------------------------------------
// dense real arrays <-> the haloed (Center, Center, Center) field, and the one-column buffers of the partitioned model's fused step
// ---------------------------------------------------------------------------------------------------------------------
// dense x-fastest real array, cell (i, j, k) at (i-1) + sj (j-1) + sk (k-1), -> interior of the field (copy_real_component!,
// fft_based_poisson_solver.jl:129-137, where a solver's inverse transform cannot write into the field itself)
__global__ void __launch_bounds__(256) copy_dense_to_field_kernel(DGrid g, FView phi, const double *src, long sj, long sk) {
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x;
    const int j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    const int k = 1 + blockIdx.z;
    if (i > g.Nx || j > g.Ny || k > g.Nz) return;
    phi.at(i, j, k) = src[(long)(i - 1) + sj * (j - 1) + sk * (k - 1)];
}

// dense z-fastest real array r[(k-1) + Nz ((i-1) + Nx (j-1))] -> interior of the field, transposed through an LDS tile
__global__ void __launch_bounds__(256) copy_real_zfast_kernel(DGrid g, FView p, const double *r) {
    __shared__ double tile[32][33];
    const int i0 = 1 + blockIdx.x * 32, k0 = 1 + blockIdx.y * 32, j = 1 + blockIdx.z;
    const int tx = threadIdx.x, ty = threadIdx.y;
    for (int ii = ty; ii < 32; ii += 8) {
        const int k = k0 + tx, i = i0 + ii;
        if (i <= g.Nx && k <= g.Nz) tile[ii][tx] = r[(long)(k - 1) + (long)g.Nz * ((i - 1) + (long)g.Nx * (j - 1))];
    }
    __syncthreads();
    for (int kk = ty; kk < 32; kk += 8) {
        const int i = i0 + tx, k = k0 + kk;
        if (i <= g.Nx && k <= g.Nz) p.at(i, j, k) = tile[tx][kk];
    }
}

// one interior column of a haloed field -> dense (Ny, Nz) buffers: west[j-1 + Ny (k-1)] = f[iw, j, k], east[...] = f[ie, j, k]
__global__ void __launch_bounds__(256) column_pack_kernel(DGrid g, FView f, int iw, int ie, double *west, double *east) {
    const int j = 1 + blockIdx.x * blockDim.x + threadIdx.x, k = 1 + blockIdx.y;
    if (j > g.Ny || k > g.Nz) return;
    const long b = (long)(j - 1) + (long)g.Ny * (k - 1);
    west[b] = f.at(iw, j, k);
    east[b] = f.at(ie, j, k);
}
// the same from the z-fastest dense real array r[(k-1) + Nz ((i-1) + Nx (j-1))]: buffers laid out [k-1 + Nz (j-1)]
__global__ void __launch_bounds__(256) column_pack_zfast_kernel(int Nx, int Ny, int Nz, const double *r, double *west, double *east) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
    if (k >= Nz || j >= Ny) return;
    const long b = (long)k + (long)Nz * j;
    west[b] = r[(long)k + (long)Nz * (0 + (long)Nx * j)];
    east[b] = r[(long)k + (long)Nz * ((Nx - 1) + (long)Nx * j)];
}
// first / last column of the dense x-fastest array -> dense (Ny, Nz) buffers [j-1 + Ny (k-1)]
__global__ void __launch_bounds__(256) column_pack_dense_kernel(int Nx, int Ny, int Nz, const double *r, double *west, double *east, long sj, long sk) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    if (j >= Ny || k >= Nz) return;
    const long row = sj * j + sk * k, b = (long)j + (long)Ny * k;
    west[b] = r[row];
    east[b] = r[row + Nx - 1];
}

// ---------------------------------------------------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------------------------------------------------
// how a dense x-fastest real array holds cell (i, j, k): at (i-1) + sj (j-1) + sk (k-1); (0, 0) stands for the fields' own order (Nx, Nx Ny)
struct DenseLayout {
    long sj = 0, sk = 0;
    DenseLayout on(const DGrid &g) const { return sj ? *this : DenseLayout{(long)g.Nx, (long)g.Nx * g.Ny}; }
};
// where a solver leaves its dense solution
struct DenseSolution { const double *p; DenseLayout at; };
// where the source term goes and what it reads: `pad`: rows of odd Nx get one zero behind them; `wrap`: the mask of source_value;
// `u_east`: the received column u[Nx + 1] of a partitioned slab
struct SourceLayout {
    DenseLayout at;
    bool pad = false;
    int wrap = 0;
    const double *u_east = nullptr;
};

static int source_term(const DGrid &g, const double *u, const double *v, const double *w, void *rhs, bool weight, bool real_out = false,
                       const SourceLayout &to = SourceLayout()) {
    const DenseLayout at = to.at.on(g);
    if (real_out)
        hipLaunchKernelGGL(source_term_kernel<true>, grid3(g.Nx, g.Ny, g.Nz, BLK), BLK, 0, g_stream, g, make_view(g, u, LOC_U),
                           make_view(g, v, LOC_V), make_view(g, w, LOC_W), rhs, weight, at.sj, at.sk, to.pad, to.wrap, to.u_east);
    else
        hipLaunchKernelGGL(source_term_kernel<false>, grid3(g.Nx, g.Ny, g.Nz, BLK), BLK, 0, g_stream, g, make_view(g, u, LOC_U),
                           make_view(g, v, LOC_V), make_view(g, w, LOC_W), rhs, weight, at.sj, at.sk, false);
    KERNEL_CHECK();
    return OCN_OK;
}

// into the z-fastest dense real array (source_term_zfast_kernel); u_east: the fused step's form, no halo read
static int source_term_zfast(const DGrid &g, const double *u, const double *v, const double *w, double *r, const double *u_east = nullptr) {
    hipLaunchKernelGGL(source_term_zfast_kernel, dim3((g.Nx + 31) / 32, (g.Nz + 31) / 32, g.Ny), dim3(32, 8), 0, g_stream, g, make_view(g, u, LOC_U),
                       make_view(g, v, LOC_V), make_view(g, w, LOC_W), u_east ? 6 : 0, u_east, r);
    KERNEL_CHECK();
    return OCN_OK;
}

static int pressure_correction(const DGrid &g, double *u, double *v, double *w, const double *p, const int *range = nullptr,
                               double *pdiv = nullptr, double divisor = 1.0) {
    Range6 r{1, g.Nx, 1, g.Ny, 1, g.Nz};
    if (range) {
        const int N[3] = {g.Nx, g.Ny, g.Nz};
        for (int d = 0; d < 3; ++d)
            if (range[2 * d] < 1 || range[2 * d + 1] > N[d])
                return fail(OCN_EINVAL, "range [%d, %d] along dimension %d leaves the interior", range[2 * d], range[2 * d + 1], d);
        r = Range6{range[0], range[1], range[2], range[3], range[4], range[5]};
    }
    const int nx = r.i1 - r.i0 + 1, ny = r.j1 - r.j0 + 1, nz = r.k1 - r.k0 + 1;
    if (nx <= 0 || ny <= 0 || nz <= 0) return OCN_OK;
    const dim3 blk = nx < 16 ? dim3(4, 64, 1) : BLK;        // an Hx-wide boundary strip: threads along y instead of 61 idle lanes in x
    hipLaunchKernelGGL(pressure_correction_kernel, grid3(nx, ny, nz, blk), blk, 0, g_stream, g, make_view(g, u, LOC_U),
                       make_view(g, v, LOC_V), make_view(g, w, LOC_W), make_view(g, p, LOC_C), r, pdiv, divisor);
    KERNEL_CHECK();
    return OCN_OK;
}

// the correction from a dense x-fastest solution on the columns ia .. ib (a Bounded z: the no-flux rule); pw: the received west column of a
// partitioned slab, NULL: x wraps. The caller checks the launch.
static void launch_pressure_correction_dense(const DGrid &g, double *u, double *v, double *w, const DenseSolution &d, const double *pw, double *p,
                                             double divisor, bool store_p, int ia, int ib) {
    const DenseLayout at = d.at.on(g);
    hipLaunchKernelGGL(pressure_correction_dense_slab_kernel, grid3(ib - ia + 1, g.Ny, g.Nz, BLK), BLK, 0, g_stream, g, make_view(g, u, LOC_U),
                       make_view(g, v, LOC_V), make_view(g, w, LOC_W), d.p, pw, make_view(g, p, LOC_C), divisor, ia, ib, at.sj, at.sk,
                       g.tz != OCN_PERIODIC, store_p);
}

static int divide_interior(const DGrid &g, double *p, double divisor) {
    hipLaunchKernelGGL(divide_interior_kernel, grid3(g.Nx, g.Ny, g.Nz, BLK), BLK, 0, g_stream, g, make_view(g, p, LOC_C), divisor);
    KERNEL_CHECK();
    return OCN_OK;
}

// dense x-fastest real array -> interior of the haloed field. The caller checks the launch.
static void launch_copy_dense_to_field(const DGrid &g, double *phi, const DenseSolution &d) {
    const DenseLayout at = d.at.on(g);
    hipLaunchKernelGGL(copy_dense_to_field_kernel, grid3(g.Nx, g.Ny, g.Nz, BLK), BLK, 0, g_stream, g, make_view(g, phi, LOC_C), d.p, at.sj, at.sk);
}
