// ocn_boundary_conditions.h -- boundary conditions (src/BoundaryConditions): the halo fills, the Flux conditions applied to a tendency and
// the halo buffers of partitioned runs, kernels first, then the host launchers of the fills and the Flux conditions. Included by
// ocn_api.hip ahead of everything that fills a halo; the launchers of the halo buffers are in ocn_dist.h and ocn_dist_poisson.h.
//
// ONE implementation of each expression:
//   * wrapped             the interior source of a parent index along a Periodic direction -- every kernel that wraps reads there;
//   * wall_halo_value     the first halo cell of a Center field on a wall: mirror, Value, Gradient;
//   * open_wall_value     the wall face of a Face field: the Open value or 0;
//   * add_flux_condition, linear_flux (ocn_device.h: the tendency epilogues of ocn_kernels.h apply them too)   G ± flux A / V, a + b φ.
// Copies and fixed formulas on the same operands in the same order on every path (the build has -ffp-contract=off): the same bits.
#pragma once
#include "ocn_device.h"
#include <array>

// 0-based parent index of the interior cell that parent index i of a Periodic direction (interior [H, H + N)) is an image of.
// N >= H (ocn_grid_create refuses anything else in a non-Flat direction), so one step reaches the interior and no caller tests it.
// A direction passed as H = 0, N = P (not Periodic, or not filled by this launch) makes every index its own source.
__device__ __forceinline__ int wrapped(int i, int H, int N) { return i < H ? i + N : (i >= H + N ? i - N : i); }

// ---------------------------------------------------------------------------------------------------------------------
// halo fills. One launch handles up to OCN_MAX_FIELDS fields of identical parent shape (FieldList, ocn_device.h).
// ---------------------------------------------------------------------------------------------------------------------
// Periodic directions: the directional fills _fill_periodic_*_halo! (fill_halo_regions_periodic.jl:5-33; parent[i] = parent[N+i],
// parent[N+H+i] = parent[H+i] for i = 1..H, over the whole extent of the two other dims) of up to three directions in ONE launch.
// Filling z, then y, then x over the whole parent extent (the reference's order) leaves every halo cell -- edges and corners
// included -- equal to the interior cell at the wrapped index in each direction, so each halo cell can be written directly from that
// interior cell: same bits, a third of the launches, and the x halos are no longer a separate uncoalesced pass. A direction that this
// launch does not fill is passed as H = 0, N = P. Thread -> one halo cell of the (P0, P1, P2) parent.
__global__ void __launch_bounds__(256) fill_periodic_xyz_kernel(FieldList fl, int P0, int P1, int P2, int N0, int N1, int N2, int H0,
                                                                int H1, int H2) {
    // halo cells are enumerated as three slabs: all (i, j) of the 2*H2 halo planes; then, for interior k, the 2*H1 halo rows;
    // then, for interior (j, k), the 2*H0 halo columns
    const long nz = (long)P0 * P1 * (2 * H2), ny = (long)P0 * (2 * H1) * N2, nx = (long)(2 * H0) * N1 * N2;
    long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    int i, j, k;
    if (t < nz) {
        i = t % P0; const long r = t / P0; j = r % P1; const int hz = r / P1;
        k = hz < H2 ? hz : N2 + hz;
    } else if ((t -= nz) < ny) {
        i = t % P0; const long r = t / P0; const int hy = r % (2 * H1);
        j = hy < H1 ? hy : N1 + hy;
        k = H2 + (int)(r / (2 * H1));
    } else if ((t -= ny) < nx) {
        const int hx = t % (2 * H0); const long r = t / (2 * H0);
        i = hx < H0 ? hx : N0 + hx;
        j = H1 + (int)(r % N1);
        k = H2 + (int)(r / N1);
    } else return;
    const long od = i + (long)P0 * (j + (long)P1 * k), os = wrapped(i, H0, N0) + (long)P0 * (wrapped(j, H1, N1) + (long)P1 * wrapped(k, H2, N2));
    for (int f = 0; f < fl.n; ++f) fl.p[f][od] = fl.p[f][os];
}

// The conditions of the fields of a FieldList on the two walls of one direction
#define OCN_BC_OPEN_SCHEME 5          // internal: an Open side that carries a scheme (ocn_open_boundary.h); never crosses the C ABI
struct BcSides {
    int kind[OCN_MAX_FIELDS][2];      // [field][lo | hi], OCN_BC_*
    double value[OCN_MAX_FIELDS][2];
    const double *arr[OCN_MAX_FIELDS][2];   // array-valued condition (getbc(::AbstractArray, i, j), boundary_condition.jl:164) or null
    double dlo, dhi;                  // spacing at the boundary faces (Δ between the first interior and the first halo point)
    // the condition at tangential interior point (a, b) (1-based) of a dense (Na, .) array, or the number
    __device__ __forceinline__ double get(int f, int side, long ab) const {
        const double *p = arr[f][side];
        return p ? p[ab] : value[f][side];
    }
};

// Center fields: the first halo cell beyond wall `side` from the adjacent interior cell c. Flux / default -> mirror
// (fill_halo_regions_flux.jl:9-27); Value / Gradient -> linear extrapolation through the boundary face
// (fill_halo_regions_value_gradient.jl:7-119)
__device__ __forceinline__ double wall_halo_value(const BcSides &bc, int f, int side, double c, long ab) {
    const int kind = bc.kind[f][side];
    if (kind == OCN_BC_VALUE) return side ? c + ((bc.get(f, 1, ab) - c) / (bc.dhi / 2)) * bc.dhi : c + ((c - bc.get(f, 0, ab)) / (bc.dlo / 2)) * (-bc.dlo);
    if (kind == OCN_BC_GRADIENT) return c + bc.get(f, side, ab) * (side ? bc.dhi : -bc.dlo);
    return c;
}
// Face fields: the value on the wall face (fill_halo_regions_open.jl:2-7; impenetrable = 0)
__device__ __forceinline__ double open_wall_value(const BcSides &bc, int f, int side, long ab) {
    return bc.kind[f][side] == OCN_BC_OPEN ? bc.get(f, side, ab) : 0.0;
}

// Bounded directions, ONE halo cell (fill_halo_kernels.jl:69-70), launched over the INTERIOR extent (grid N) of the two
// other dims; Face fields are skipped when fill_open_bcs = false.
// ea_lo / ea_hi (z fill of an x-slab rank's DIFFUSIVITY fields only): also fill the first halo column on a connected x side -- the rank
// evaluates the eddy diffusivities at i = 0 / Nx + 1 itself, and a serial Periodic run's x fill copies the z-filled value into those
// cells (the closure's corner interpolations at the rank edge read them); an array-valued condition is read at the nearest interior point
template <int D>
__global__ void __launch_bounds__(256) fill_bounded_kernel(FieldList fl, BcSides bc, FView view, int Na, int Nb, int N, bool face,
                                                           bool fill_open, bool do_lo = true, bool do_hi = true, int ea_lo = 0, int ea_hi = 0) {   // one-sided: Left / RightConnected x
    long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int Nae = Na + ea_lo + ea_hi;
    if (t >= (long)Nae * Nb) return;
    int a = 1 - ea_lo + t % Nae, b = 1 + t / Nae;
    long lo, ilo, hi, ihi;
    if (D == 0) { lo = view.lin(face ? 1 : 0, a, b); ilo = view.lin(1, a, b); hi = view.lin(N + 1, a, b); ihi = view.lin(N, a, b); }
    else if (D == 1) { lo = view.lin(a, face ? 1 : 0, b); ilo = view.lin(a, 1, b); hi = view.lin(a, N + 1, b); ihi = view.lin(a, N, b); }
    else { lo = view.lin(a, b, face ? 1 : 0); ilo = view.lin(a, b, 1); hi = view.lin(a, b, N + 1); ihi = view.lin(a, b, N); }
    const long ab = (long)(min(max(a, 1), Na) - 1) + (long)Na * (b - 1);
    for (int f = 0; f < fl.n; ++f) {
        double *p = fl.p[f];
        if (!face) {
            const double h0 = wall_halo_value(bc, f, 0, p[ilo], ab), h1 = wall_halo_value(bc, f, 1, p[ihi], ab);
            if (do_lo) p[lo] = h0;
            if (do_hi) p[hi] = h1;
        } else if (fill_open) {
            // a side with a scheme is left alone: its boundary value is the scheme's state, stepped by open_boundary_step_kernel
            if (do_lo && bc.kind[f][0] != OCN_BC_OPEN_SCHEME) p[lo] = open_wall_value(bc, f, 0, ab);
            if (do_hi && bc.kind[f][1] != OCN_BC_OPEN_SCHEME) p[hi] = open_wall_value(bc, f, 1, ab);
        }
    }
}

// (Periodic | FullyConnected, Periodic, Bounded) grids: the bounded z fill and the periodic y and x fills in ONE launch. The reference
// fills z first (one halo cell below and above, over the interior (i, j) only), then y, then x over the whole extent of the other
// dimensions (boundary_condition_ordering.jl:17-46), which leaves
//   * the two z-boundary planes (Center fields: k = 0 and N+1; Face fields: the wall planes k = 1 and N+1) holding, at EVERY (i, j) of
//     the parent, the boundary formula evaluated in the column at the wrapped interior (i, j);
//   * every other plane -- the deeper z halos included, whose interior (i, j) nobody writes -- holding in its x / y halo cells the
//     value of the wrapped interior (i, j) of the same plane.
// Each such cell is written here directly from those sources: same bits, a third of the launches. `zfill`: the z fill runs (Center
// fields always; Face fields when fill_open_bcs). An x-slab rank (x halos owned by the neighbours) passes H0 = 0, N0 = P0 and XC = Hx:
// its XC outermost columns are left to the exchange -- in the z-boundary planes they only take part in the periodic y copy.
// XZ (diffusivity fields of an x-slab rank, see fill_bounded_kernel): the innermost XZ of the XC neighbour columns take the z formula too.
// Never launched for fields with a scheme on bottom or top (fill_halo_group sends those through fill_bounded_kernel, which leaves such
// a side alone): open_wall_value is the whole Face rule here.
__global__ void __launch_bounds__(256) fill_periodic_xy_bounded_z_kernel(FieldList fl, BcSides bc, int P0, int P1, int P2, int N0, int N1,
                                                                         int N2, int H0, int H1, int H2, bool face, bool zfill, int XC,
                                                                         int NA, int XZ = 0) {
    const int klo = face ? H2 : H2 - 1, khi = N2 + H2;                       // 0-based parent planes of the z fill
    const long nA = zfill ? (long)P0 * P1 * 2 : 0;
    const int nplanes = P2 - (zfill ? 2 : 0);
    const long rowsB = (long)P0 * (2 * H1), colsB = (long)(2 * H0) * N1, perplane = rowsB + colsB;
    long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < nA) {
        const int i = t % P0; const long r = t / P0; const int j = r % P1; const int side = r / P1;
        const int si = wrapped(i, H0, N0), sj = wrapped(j, H1, N1);
        const long col = si + (long)P0 * sj, plane = (long)P0 * P1;
        const long od = i + (long)P0 * j + plane * (side ? khi : klo);
        if (i < XC - XZ || i >= P0 - XC + XZ) {                             // a neighbour's column: periodic y copy only
            if (sj == j) return;
            const long os = col + plane * (side ? khi : klo);
            for (int f = 0; f < fl.n; ++f) fl.p[f][od] = fl.p[f][os];
            return;
        }
        const long ab = (long)min(max(si - H0 - XC, 0), NA - 1) + (long)NA * (sj - H1);      // tangential interior point (i, j) of the source column
        const long oc = col + plane * (side ? N2 + H2 - 1 : H2);                            // first / last interior cell of the column
        for (int f = 0; f < fl.n; ++f) {
            double *p = fl.p[f];
            p[od] = face ? open_wall_value(bc, f, side, ab) : wall_halo_value(bc, f, side, p[oc], ab);
        }
        return;
    }
    t -= nA;
    if (t >= perplane * nplanes) return;
    int kp = (int)(t / perplane);
    if (zfill) { if (kp >= klo) ++kp; if (kp >= khi) ++kp; }
    long q = t % perplane;
    int i, j;
    if (q < rowsB) { i = q % P0; const int hy = q / P0; j = hy < H1 ? hy : N1 + hy; }
    else { q -= rowsB; const int hx = q % (2 * H0); i = hx < H0 ? hx : N0 + hx; j = H1 + (int)(q / (2 * H0)); }
    const long plane = (long)P0 * P1 * kp;
    const long od = i + (long)P0 * j + plane, os = wrapped(i, H0, N0) + (long)P0 * wrapped(j, H1, N1) + plane;
    for (int f = 0; f < fl.n; ++f) fl.p[f][od] = fl.p[f][os];
}

// ---------------------------------------------------------------------------------------------------------------------
// Flux conditions on a tendency (compute_flux_bcs.jl:57-163), over the interior extent of the two other dims of direction D
// ---------------------------------------------------------------------------------------------------------------------
// compute_x/y/z_bcs!: G[1] += flux * A / V, G[N] -= flux * A / V; alo / ahi: array-valued conditions (null: the numbers flo / fhi)
template <int D>
__global__ void __launch_bounds__(256) flux_bc_kernel(DGrid g, FView G, int Na, int Nb, int N, int lz, bool has_lo, double flo, bool has_hi,
                                                      double fhi, const double *alo, const double *ahi) {
    long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long)Na * Nb) return;
    const int a = 1 + t % Na, b = 1 + t / Na;
    for (int side = 0; side < 2; ++side) {
        if (side == 0 ? !has_lo : !has_hi) continue;
        const int n = side ? N : 1;
        const int i = D == 0 ? n : a, j = D == 1 ? n : (D == 0 ? a : b), k = D == 2 ? n : b;
        const double *arr = side ? ahi : alo;
        const double flux = arr ? arr[(long)(a - 1) + (long)Na * (b - 1)] : (side ? fhi : flo);
        double &Gq = G.at(i, j, k);
        Gq = add_flux_condition(g, D, lz, k, side, flux, Gq);
    }
}

// One side of a field-dependent Flux condition of the linear family: flux = a + b φ[i, j, k_boundary] (φ at the location of the field
// that carries the condition => identity interpolation), applied like the valued Flux above.
template <int D>
__global__ void __launch_bounds__(256) linear_flux_bc_kernel(DGrid g, FView G, FView P, int Na, int Nb, int N, int lz, int side, double a_,
                                                             double b_) {
    long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long)Na * Nb) return;
    const int a = 1 + t % Na, b = 1 + t / Na;
    const int n = side ? N : 1;
    const int i = D == 0 ? n : a, j = D == 1 ? n : (D == 0 ? a : b), k = D == 2 ? n : b;
    double &Gq = G.at(i, j, k);
    Gq = add_flux_condition(g, D, lz, k, side, linear_flux(a_, b_, P.at(i, j, k)), Gq);
}

// ---------------------------------------------------------------------------------------------------------------------
// halo buffers of partitioned runs (src/DistributedComputations)
// ---------------------------------------------------------------------------------------------------------------------
// fill_send_buffers! / recv_from_buffers! for a 1-D x partition (communication_buffers.jl:281-313): the west / east
// buffers hold Hx x Py x Pz slabs -- the whole parent extent in y and z, so corners ride along (:53,71-76).
// PACK: west_send <- parent[Hx .. 2Hx), east_send <- parent[Nx .. Nx+Hx);  UNPACK: parent[0 .. Hx) <- west_recv,
// parent[Nx+Hx .. Nx+2Hx) <- east_recv. Buffers are field-major; field f (its own Py x Pz: Face fields on Bounded
// dimensions have one more plane) starts at off[f] and holds rows[f] = Py*Pz rows of Hx values.
struct SlabList {
    long off[OCN_MAX_FIELDS];
    long rows[OCN_MAX_FIELDS];
    int p0[OCN_MAX_FIELDS];                    // parent extent in x of each field
};
template <bool PACK>
__global__ void __launch_bounds__(256) x_halo_buffer_kernel(FieldList fl, SlabList sl, int N, int HX, int H, double *west, double *east,
                                                            bool do_west, bool do_east) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int h = t % H;
    const long r = t / H;                      // j + P1 * k
    for (int f = 0; f < fl.n; ++f) {
        if (r >= sl.rows[f]) continue;
        double *p = fl.p[f];
        const long row = r * sl.p0[f];
        const long b = sl.off[f] + t;
        // H = exchanged depth (<= Hx = HX): the depth interior columns next to each side <-> the depth halo columns nearest to it
        if (PACK) {
            west[b] = p[row + HX + h];
            east[b] = p[row + HX + N - H + h];
        } else {
            if (do_west) p[row + HX - H + h] = west[b];
            if (do_east) p[row + N + HX + h] = east[b];
        }
    }
}

// fill_send_buffers! of x_halo_buffer_kernel<true> with the y / z halo rows read at their WRAPPED interior source (y, z Periodic, every
// field with parent extents (Px, Ny + 2Hy, Nz + 2Hz)): what the buffers would hold after a local fill of the packed columns
__global__ void __launch_bounds__(256) x_halo_pack_wrapped_kernel(FieldList fl, SlabList sl, int N, int HX, int H, int Ny, int Hy, int Nz, int Hz,
                                                                  double *west, double *east) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int h = t % H;
    const long r = t / H;                      // j + P1 * k over the parent extents
    const int P1 = Ny + 2 * Hy;
    const int jp = (int)(r % P1), kp = (int)(r / P1);
    if (kp >= Nz + 2 * Hz) return;
    const int js = wrapped(jp, Hy, Ny), ks = wrapped(kp, Hz, Nz);
    for (int f = 0; f < fl.n; ++f) {
        const double *p = fl.p[f];
        const long row = ((long)js + (long)P1 * ks) * sl.p0[f];
        const long b = sl.off[f] + t;
        west[b] = p[row + HX + h];
        east[b] = p[row + HX + N - H + h];
    }
}

// the same along y for pencil partitions: the south / north buffers hold Hy rows of the WHOLE parent extent in x and z, so the x halos
// just received -- the corners of halo_communication.jl:137-162 -- ride along on the second hop
struct RowList {
    long off[OCN_MAX_FIELDS];
    int p0[OCN_MAX_FIELDS], p1[OCN_MAX_FIELDS], p2[OCN_MAX_FIELDS];
};
template <bool PACK>
__global__ void __launch_bounds__(256) y_halo_buffer_kernel(FieldList fl, RowList rl, int N, int HY, int H, double *south, double *north,
                                                            bool do_south, bool do_north) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    for (int f = 0; f < fl.n; ++f) {
        const int p0 = rl.p0[f];
        const long per = (long)p0 * H;
        if (t >= per * rl.p2[f]) continue;
        const int i = t % p0, h = (t / p0) % H;
        const long k = t / per;
        double *p = fl.p[f];
        const long base = i + (long)p0 * (long)rl.p1[f] * k;
        const long b = rl.off[f] + t;
        if (PACK) {
            south[b] = p[base + (long)p0 * (HY + h)];
            north[b] = p[base + (long)p0 * (HY + N - H + h)];
        } else {
            if (do_south) p[base + (long)p0 * (HY - H + h)] = south[b];
            if (do_north) p[base + (long)p0 * (N + HY + h)] = north[b];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------------------------------------------------
// the conditions of n fields on the two walls of direction d; bcs == nullptr: all default
static BcSides bc_sides(const ocn_bc_t (*bcs)[6], int n, int d, const ocn_grid_s *grid) {
    const DGrid &g = grid->d;
    BcSides bc;
    for (int f = 0; f < n; ++f)
        for (int sd = 0; sd < 2; ++sd) {
            bc.kind[f][sd] = bcs ? bcs[f][2 * d + sd].kind : OCN_BC_DEFAULT;
            bc.value[f][sd] = bcs ? bcs[f][2 * d + sd].value : 0.0;
            bc.arr[f][sd] = bcs ? bcs[f][2 * d + sd].array : nullptr;
        }
    // Δ at the boundary faces (flip(Center) = Face): Δxᶠ = Δx, Δyᶠ = Δy, Δzᶠ[1], Δzᶠ[N+1]
    bc.dlo = d == 0 ? g.dx : (d == 1 ? g.dy : grid->h_dzf[g.Hz]);
    bc.dhi = d == 0 ? g.dx : (d == 1 ? g.dy : grid->h_dzf[g.Nz + g.Hz]);
    return bc;
}

static int fill_halo_group(const OcnOptions &o, const ocn_grid_s *grid, double *const *fields, int n, const int loc[3], bool fill_open,
                           const ocn_bc_t (*bcs)[6], bool extend_x = false) {
    if (n <= 0) return OCN_OK;
    const DGrid &g = grid->d;
    FieldList fl;
    fl.n = n;
    for (int f = 0; f < n; ++f) fl.p[f] = fields[f];
    int P[3];
    parent_size(g, loc, P);
    const int N[3] = {g.Nx, g.Ny, g.Nz}, H[3] = {g.Hx, g.Hy, g.Hz}, T[3] = {g.tx, g.ty, g.tz};
    FView view = make_view(g, nullptr, loc);
    // a side with a scheme (bottom / top of w) is skipped by the bounded fill; the fused kernel below has no such case
    bool scheme_side = false;
    for (int f = 0; bcs && f < n; ++f)
        for (int sd = 0; sd < 6; ++sd) scheme_side = scheme_side || bcs[f][sd].kind == OCN_BC_OPEN_SCHEME;
    // (Periodic | FullyConnected, Periodic, Bounded): bounded z fill + periodic y and x fills as one launch
    if (!scheme_side && o.fused_halo && (T[0] == OCN_PERIODIC || T[0] == OCN_CONNECTED) && T[1] == OCN_PERIODIC && T[2] == OCN_BOUNDED) {
        const bool face = loc[2] == OCN_FACE, zfill = !face || fill_open, slab = T[0] == OCN_CONNECTED;
        const int H0 = slab ? 0 : H[0], N0 = slab ? P[0] : N[0];
        const long total = (zfill ? (long)P[0] * P[1] * 2 : 0) + ((long)P[0] * (2 * H[1]) + (long)(2 * H0) * N[1]) * (P[2] - (zfill ? 2 : 0));
        hipLaunchKernelGGL(fill_periodic_xy_bounded_z_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, g_stream, fl,
                           bc_sides(bcs, n, 2, grid), P[0], P[1], P[2], N0, N[1], N[2], H0, H[1], H[2], face, zfill, slab ? H[0] : 0, N[0],
                           extend_x && slab ? 1 : 0);
        KERNEL_CHECK();
        return OCN_OK;
    }
    // order: boundary_condition_ordering.jl:17-46 -- non-periodic first, then periodic; insertion sort with an
    // always-true `lt` reverses same-class entries => z, y, x inside each class.
    // (a kernel templated on the direction is launched through the table of its three instantiations)
    const auto bounded = std::array{fill_bounded_kernel<0>, fill_bounded_kernel<1>, fill_bounded_kernel<2>};
    for (int d = 2; d >= 0; --d) {
        const bool do_lo = wall_lo(T[d]), do_hi = wall_hi(T[d]);            // one wall only on Right / LeftConnected x, y
        if (!do_lo && !do_hi) continue;
        const bool face = loc[d] == OCN_FACE;
        if (face && !fill_open) continue;
        const int Na = d == 0 ? N[1] : N[0], Nb = d == 2 ? N[1] : N[2];
        // connected x sides of an x-slab rank's diffusivity fields: the first halo column takes the z fill too (see fill_bounded_kernel)
        const int el = d == 2 && extend_x && (T[0] == OCN_CONNECTED || T[0] == OCN_LEFT_CONNECTED) ? 1 : 0;
        const int eh = d == 2 && extend_x && (T[0] == OCN_CONNECTED || T[0] == OCN_RIGHT_CONNECTED) ? 1 : 0;
        const int nb = (int)(((long)(Na + el + eh) * Nb + 255) / 256);
        hipLaunchKernelGGL(bounded[d], dim3(nb), dim3(256), 0, g_stream, fl, bc_sides(bcs, n, d, grid), view, Na, Nb, N[d], face, fill_open, do_lo,
                           do_hi, el, eh);
    }
    // Periodic directions: one launch writes every halo cell of the directions in `dirs` (bit d) from its wrapped interior source; a
    // direction left out -- a wall, a Flat one, the x of an x-slab rank, whose x halos come from the neighbours -- is its own source
    // over its whole extent
    auto fill_periodic = [&](int dirs) {
        int Nd[3], Hd[3];
        for (int d = 0; d < 3; ++d) {
            const bool fill = ((dirs >> d) & 1) && T[d] == OCN_PERIODIC;
            Hd[d] = fill ? H[d] : 0;
            Nd[d] = fill ? N[d] : P[d];
        }
        const long total = (long)P[0] * P[1] * (2 * Hd[2]) + (long)P[0] * (2 * Hd[1]) * Nd[2] + (long)(2 * Hd[0]) * Nd[1] * Nd[2];
        if (total)
            hipLaunchKernelGGL(fill_periodic_xyz_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, g_stream, fl, P[0], P[1], P[2], Nd[0],
                               Nd[1], Nd[2], Hd[0], Hd[1], Hd[2]);
    };
    // fused_halo = 0: the reference's directional fills z, y, x, each reading what the previous one wrote
    if (o.fused_halo) fill_periodic(7);
    else for (int d = 2; d >= 0; --d) fill_periodic(1 << d);
    KERNEL_CHECK();
    return OCN_OK;
}

// FieldBoundaryConditions validation: Bounded sides only; Flux / Value / Gradient on fields at Center along the boundary
// direction, Open on the wall-normal (Face) component
static int validate_bc(const DGrid &g, const int loc[3], int side, int kind) {
    const int T[3] = {g.tx, g.ty, g.tz};
    if (side < 0 || side > 5) return fail(OCN_EINVAL, "side %d out of range (0..5 = west, east, south, north, bottom, top)", side);
    if (kind < OCN_BC_DEFAULT || kind > OCN_BC_OPEN) return fail(OCN_EINVAL, "unknown boundary condition kind %d", kind);
    if (kind == OCN_BC_DEFAULT) return OCN_OK;
    const int d = side / 2;
    if (!((side & 1) ? wall_hi(T[d]) : wall_lo(T[d])))
        return fail(OCN_EINVAL, "a non-default boundary condition needs a wall on that side (Bounded topology) in dimension %d", d);
    if (kind == OCN_BC_OPEN ? loc[d] != OCN_FACE : loc[d] != OCN_CENTER)
        return fail(OCN_EINVAL, "Flux/Value/Gradient conditions apply to fields at Center, Open to fields at Face along the boundary direction");
    return OCN_OK;
}

// groups fields by identical location (identical parent shape) -> one set of launches per group
static int fill_halo_regions(const OcnOptions &o, const ocn_grid_s *grid, double *const *fields, const int (*locs)[3], int nfields, bool fill_open,
                             const ocn_bc_t (*bcs)[6] = nullptr, bool extend_x = false) {
    const DGrid &g = grid->d;
    if (nfields > OCN_MAX_FIELDS) return fail(OCN_EINVAL, "at most %d fields per call", OCN_MAX_FIELDS);
    bool done[OCN_MAX_FIELDS] = {false};
    for (int f = 0; f < nfields; ++f) {
        if (done[f]) continue;
        double *grp[OCN_MAX_FIELDS];
        ocn_bc_t gbc[OCN_MAX_FIELDS][6];
        int n = 0;
        int P0[3], P1[3];
        parent_size(g, locs[f], P0);
        for (int h = f; h < nfields; ++h) {
            if (done[h]) continue;
            parent_size(g, locs[h], P1);
            bool same = P0[0] == P1[0] && P0[1] == P1[1] && P0[2] == P1[2];
            for (int d = 0; d < 3 && same; ++d) {
                const int T[3] = {g.tx, g.ty, g.tz};
                if ((wall_lo(T[d]) || wall_hi(T[d])) && locs[h][d] != locs[f][d]) same = false;
            }
            if (same) {
                if (bcs) memcpy(gbc[n], bcs[h], sizeof(ocn_bc_t) * 6);
                grp[n++] = fields[h];
                done[h] = true;
            }
        }
        int rc = fill_halo_group(o, grid, grp, n, locs[f], fill_open, bcs ? gbc : nullptr, extend_x);
        if (rc) return rc;
    }
    return OCN_OK;
}

static int compute_flux_bcs(const DGrid &g, double *G, const int loc[3], const ocn_bc_t bcs[6]) {
    const int N[3] = {g.Nx, g.Ny, g.Nz}, T[3] = {g.tx, g.ty, g.tz};
    const auto kernel = std::array{flux_bc_kernel<0>, flux_bc_kernel<1>, flux_bc_kernel<2>};
    FView view = make_view(g, G, loc);
    for (int d = 0; d < 3; ++d) {
        const bool lo = wall_lo(T[d]) && bcs[2 * d].kind == OCN_BC_FLUX, hi = wall_hi(T[d]) && bcs[2 * d + 1].kind == OCN_BC_FLUX;
        if (!lo && !hi) continue;
        const int Na = d == 0 ? N[1] : N[0], Nb = d == 2 ? N[1] : N[2];
        const int nb = (int)(((long)Na * Nb + 255) / 256);
        hipLaunchKernelGGL(kernel[d], dim3(nb), dim3(256), 0, g_stream, g, view, Na, Nb, N[d], loc[2], lo, bcs[2 * d].value, hi, bcs[2 * d + 1].value,
                           lo ? bcs[2 * d].array : nullptr, hi ? bcs[2 * d + 1].array : nullptr);
    }
    KERNEL_CHECK();
    return OCN_OK;
}

static int compute_linear_flux_bc(const DGrid &g, double *G, const int loc[3], int side6, double a, double b, const double *dep) {
    const int N[3] = {g.Nx, g.Ny, g.Nz}, T[3] = {g.tx, g.ty, g.tz};
    const auto kernel = std::array{linear_flux_bc_kernel<0>, linear_flux_bc_kernel<1>, linear_flux_bc_kernel<2>};
    const int d = side6 / 2, side = side6 % 2;
    if (!(side ? wall_hi(T[d]) : wall_lo(T[d]))) return fail(OCN_EINVAL, "a Flux condition needs a wall on that side (Bounded direction)");
    if (loc[d] != OCN_CENTER) return fail(OCN_EINVAL, "a Flux condition needs a field at Center along the boundary direction");
    const FView vG = make_view(g, G, loc), vP = make_view(g, dep, loc);
    const int Na = d == 0 ? N[1] : N[0], Nb = d == 2 ? N[1] : N[2];
    const int nb = (int)(((long)Na * Nb + 255) / 256);
    hipLaunchKernelGGL(kernel[d], dim3(nb), dim3(256), 0, g_stream, g, vG, vP, Na, Nb, N[d], loc[2], side, a, b);
    KERNEL_CHECK();
    return OCN_OK;
}
