// ocn_diagnostics.h -- on-device diagnostics: computed fields of one BinaryOperation (AbstractOperations/binary_operations.jl,
// computed_field.jl), reductions (sum! / maximum! / minimum! / average!, Fields/field.jl:735-767, AbstractOperations/
// metric_field_reductions.jl) and accumulations (cumsum! / reverse_cumsum!, Fields/scans.jl:225-306).
//
// One evaluator, dg_eval, forms the operand at (i, j, k): loads, interpolation (Operators/interpolation_operators.jl), operation, metric,
// in that order -- the computed-field kernel, the reducing kernels and the accumulating kernels all call it, so what is summed is exactly
// what the computed field holds. It has two overloads and every kernel is a template on the operand type: DgOperand, the one fixed
// operation node, and DgStencil, a recorded stencil program (KernelFunctionOperation, Derivative, UnaryOperation) run by an interpreter.
// The translation unit is compiled with -ffp-contract=off: separate IEEE multiplies and adds.
//
// Reductions use no atomics. How the points are split into partial results depends on the grid size and the reduced directions only:
//   x reduced (dg_reduce_rows_kernel)  the (j, k) rows of one output element are cut into chunks of DG_ROWS rows, one 256-thread block per
//                                      chunk; a wave takes every fourth row of the chunk, a lane every 64th point of a row (full-wave
//                                      coalesced loads), adds them in index order; the 64 lanes combine in a shuffle tree, the four waves in
//                                      wave order. One chunk: the block writes the result. More: it stores its partial in a slab of the grid
//                                      with a plain store and dg_combine_kernel, a second small launch, adds the chunks of each output
//                                      element in one fixed order.
//   x kept (dg_reduce_cols_kernel)     one thread per output element, x across the lanes, a sequential loop over the reduced directions.
// Accumulations keep the reference's sequential order: along y and z a march per column with x across the lanes
// (dg_accumulate_cols_kernel); along x a wave per row reads 64 points at a time and every lane forms the same running sum from the lanes'
// values in index order (dg_accumulate_rows_kernel).
//
// Every kernel is also a template on WHERE it writes: DgOut, a plain store, or DgOutFold, the running time average of
// accumulate_result! (OutputWriters/windowed_time_average.jl:216-230) -- the value the plain store would write is folded into the
// element it would overwrite, in the thread that formed it (dg_store). Splits, chunks and combine orders do not depend on it.
#pragma once
#include "ocn_device.h"
#include "ocn_open_boundary.h"   // jl_min, jl_max
#include <cmath>

#define DG_THREADS 256
#define DG_ROWS 16            // rows of a chunk: 4 per wave

// one leaf of the operation: a field with its interpolation, or a number
struct DgLeaf {
    const double *p;          // nullptr: the number c
    double c;
    long off;                 // parent index of the low corner of the interpolation stencil of interior point (1, 1, 1)
    int s1;
    long s2;                  // parent strides along y and z
    int n;                    // interpolated directions (0..3)
    long st[3];               // their parent strides, innermost interpolation first
};

struct DgOperand {
    DgLeaf a, b;
    int op;                   // OCN_OP_*
    int absolute;             // f = abs
    int mmode;                // metric: 0 none, 1 mc, 2 Δz[k], 3 mc * Δz[k]
    double mc;                // Δx, Δy or Az = Δx Δy
    const double *dz;         // Δzᵃᵃᶜ or Δzᵃᵃᶠ (the operand's z location), indexed k - 1 + Hz
    int Hz;
};

// where the kernels write: parent index of output element (0, 0, 0) and strides (0 along a reduced direction)
struct DgOut {
    double *p;
    long off, s[3];
};

// the same place as the running average of a WindowedTimeAverage: result = (result * T_previous + integrand * Δt) / T_current
// (windowed_time_average.jl:224), the three times by value. first: the first sample of a window, for which advance_time_average!
// (:236-249) has just zeroed the result and T_previous is 0 -- the result is not read (no memset either) and is
// (0.0 * 0.0 + integrand * Δt) / T_current = (0.0 + integrand * Δt) / T_current, so an integrand of -0.0 gives +0.0 as it does there
struct DgOutFold : DgOut {
    double Tp, dt, Tc;
    int first;
};

__device__ __forceinline__ void dg_store(const DgOut &w, long idx, double v) { w.p[idx] = v; }
// two multiplies, one add, one correctly rounded divide, in the reference's association (-ffp-contract=off: no fma)
__device__ __forceinline__ void dg_store(const DgOutFold &w, long idx, double v) {
    const double s = v * w.dt;
    const double r = w.first ? 0.0 : w.p[idx] * w.Tp;
    w.p[idx] = (r + s) / w.Tc;
}

// ℑ of a field: 0.5 (f[low] + f[low + 1]) per direction, nested with st[0] innermost
__device__ __forceinline__ double dg_leaf(const DgLeaf &l, int i, int j, int k) {
    if (!l.p) return l.c;
    const double *q = l.p + (l.off + i + (long)l.s1 * j + l.s2 * k);
    if (l.n == 0) return q[0];
    const long s0 = l.st[0];
    if (l.n == 1) return 0.5 * (q[0] + q[s0]);
    const long s1 = l.st[1];
    if (l.n == 2) return 0.5 * (0.5 * (q[0] + q[s0]) + 0.5 * (q[s1] + q[s1 + s0]));
    const long s2 = l.st[2];
    const double lo = 0.5 * (0.5 * (q[0] + q[s0]) + 0.5 * (q[s1] + q[s1 + s0]));
    const double hi = 0.5 * (0.5 * (q[s2] + q[s2 + s0]) + 0.5 * (q[s2 + s1] + q[s2 + s1 + s0]));
    return 0.5 * (lo + hi);
}

// the metric at level k (0-based interior index)
template <class O> __device__ __forceinline__ double dg_metric(const O &o, int k) {
    if (o.mmode == 1) return o.mc;
    const double dz = o.dz[k + o.Hz];
    return o.mmode == 2 ? dz : o.mc * dz;
}

// the operand at the 0-based interior point (i, j, k): op(▶a(a), ▶b(b)) [abs] [* metric]; `metric` returns the factor (1 without one)
__device__ __forceinline__ double dg_eval(const DgOperand &o, int i, int j, int k, double &metric) {
    const double a = dg_leaf(o.a, i, j, k);
    double v = a;
    if (o.op != OCN_OP_IDENTITY) {
        const double b = dg_leaf(o.b, i, j, k);
        v = o.op == OCN_OP_ADD ? a + b : (o.op == OCN_OP_SUB ? a - b : (o.op == OCN_OP_MUL ? a * b : a / b));
    }
    if (o.absolute) v = fabs(v);
    metric = 1.0;
    if (o.mmode) {
        metric = dg_metric(o, k);
        v = v * metric;
    }
    return v;
}

// ---------------------------------------------------------------------------------------------------------------------
// stencil programs: KernelFunctionOperation (AbstractOperations/kernel_function_operation.jl:58-70), Derivative, UnaryOperation
// ---------------------------------------------------------------------------------------------------------------------
// The host records kernel_function(i, j, k, grid, args...) once as a straight-line program (ocn_stencil_ins_t) and lowers it for the
// device: every value has an LDS slot (ocn_stencil_plan: linear scan by last use), every leaf its pointer. dg_eval (the DgStencil
// overload, "dg_eval_stencil") is the ONE evaluator of such programs: the kernels below call it exactly where they call the fixed one.
// The instruction words are the same for every thread (scalar loads, a switch on a wave-uniform value); the values of a thread are
// indexed at run time, so they live in dynamic LDS, slot-major: vals[slot][thread], nslots x 256 threads x 8 B, consecutive lanes in
// consecutive banks (ocn_boundary_function.h). A thread only touches its own column: no barrier. Every instruction is ONE IEEE operation.
#define DG_ST_MAX_INS 256        // OCN_STENCIL_MAX_INSTRUCTIONS
#define DG_ST_MAX_SLOTS 64       // OCN_STENCIL_MAX_SLOTS: 64 x 2 KiB = 128 KiB of the 160 KiB of a CU
#define DG_ST_MAX_ARGS 8         // OCN_STENCIL_MAX_ARGUMENTS
#define DG_ST_LOAD 25            // p[i + s1 j + s2 k]: an argument at a constant offset (folded into p)
#define DG_ST_LINE 26            // p[i], p[j] or p[k] (c = 0, 1, 2): Δz or a node table (the offset folded into p)

struct DgStIns {
    int op;                   // OCN_EXPR_CONST, OCN_EXPR_ADD .. OCN_EXPR_SELECT, DG_ST_LOAD, DG_ST_LINE
    int a, b, c;              // SLOTS of the operands (0 where unused; DG_ST_LINE: c = the direction)
    int dst;                  // slot of the result
    int s1;
    long s2;                  // parent strides of the argument along y and z
    const double *p;
    double imm;
};

// ARITH: the program holds none of exp, log, sin, cos, tanh, pow -- an instantiation without their code (ocn_forcing_function.h)
template <bool ARITH> struct DgStencil {
    const DgStIns *ins;       // device copy of the lowered program
    int n;
    int absolute, mmode;      // as DgOperand
    double mc;
    const double *dz;
    int Hz;
};

extern __shared__ double dg_vals[];

template <bool ARITH>
__device__ __forceinline__ double dg_eval(const DgStencil<ARITH> &o, int i, int j, int k, double &metric) {
    double *vals = dg_vals + (threadIdx.y * blockDim.x + threadIdx.x);
    double r = 0.0;
    for (int q = 0; q < o.n; ++q) {
        const DgStIns I = o.ins[q];
        const double x = vals[I.a * DG_THREADS], y = vals[I.b * DG_THREADS];
        switch (I.op) {
        case OCN_EXPR_CONST: r = I.imm; break;
        case DG_ST_LOAD: r = I.p[i + (long)I.s1 * j + I.s2 * k]; break;
        case DG_ST_LINE: r = I.p[I.c == 0 ? i : (I.c == 1 ? j : k)]; break;
        case OCN_EXPR_ADD: r = x + y; break;
        case OCN_EXPR_SUB: r = x - y; break;
        case OCN_EXPR_MUL: r = x * y; break;
        case OCN_EXPR_DIV: r = x / y; break;
        case OCN_EXPR_NEG: r = -x; break;
        case OCN_EXPR_ABS: r = fabs(x); break;
        case OCN_EXPR_MIN: r = jl_min(x, y); break;
        case OCN_EXPR_MAX: r = jl_max(x, y); break;
        case OCN_EXPR_SQRT: r = sqrt(x); break;
        case OCN_EXPR_EXP: if (!ARITH) r = exp(x); break;
        case OCN_EXPR_LOG: if (!ARITH) r = log(x); break;
        case OCN_EXPR_SIN: if (!ARITH) r = sin(x); break;
        case OCN_EXPR_COS: if (!ARITH) r = cos(x); break;
        case OCN_EXPR_TANH: if (!ARITH) r = tanh(x); break;
        case OCN_EXPR_POW: if (!ARITH) r = pow(x, y); break;
        case OCN_EXPR_LT: r = x < y ? 1.0 : 0.0; break;
        case OCN_EXPR_LE: r = x <= y ? 1.0 : 0.0; break;
        case OCN_EXPR_GT: r = x > y ? 1.0 : 0.0; break;
        case OCN_EXPR_GE: r = x >= y ? 1.0 : 0.0; break;
        default: r = x != 0.0 ? y : vals[I.c * DG_THREADS]; break;          // OCN_EXPR_SELECT
        }
        vals[I.dst * DG_THREADS] = r;
    }
    double v = r;                                                          // the result is the LAST value
    if (o.absolute) v = fabs(v);
    metric = 1.0;
    if (o.mmode) {
        metric = dg_metric(o, k);
        v = v * metric;
    }
    return v;
}

// ---------------------------------------------------------------------------------------------------------------------
// computed field: _compute! (computed_field.jl:100-103)
// ---------------------------------------------------------------------------------------------------------------------
template <class O, class W>
__global__ void __launch_bounds__(256) dg_compute_kernel(O o, W out, int n0, int n1) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y, k = blockIdx.z;
    if (i >= n0 || j >= n1) return;
    double m;
    dg_store(out, out.off + i * out.s[0] + j * out.s[1] + k * out.s[2], dg_eval(o, i, j, k, m));
}

// a plain field as the integrand: the whole parent array, halos included, as `@.` on parent(result) folds it
// (windowed_time_average.jl:224)
__global__ void __launch_bounds__(256) dg_fold_parent_kernel(const double *a, DgOutFold out, long n) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < n) dg_store(out, q, a[q]);
}

// ---------------------------------------------------------------------------------------------------------------------
// reductions
// ---------------------------------------------------------------------------------------------------------------------
template <int KIND> __device__ __forceinline__ double dg_identity() {
    return KIND == OCN_REDUCE_MAXIMUM ? -INFINITY : (KIND == OCN_REDUCE_MINIMUM ? INFINITY : 0.0);
}
template <int KIND> __device__ __forceinline__ double dg_combine(double x, double y) {
    return KIND == OCN_REDUCE_MAXIMUM ? jl_max(x, y) : (KIND == OCN_REDUCE_MINIMUM ? jl_min(x, y) : x + y);
}
// sum -> s; average -> s / Σ metric or s / count; maximum, minimum -> s
template <int KIND> __device__ __forceinline__ double dg_finish(double s, double m, bool metric, double count) {
    return KIND == OCN_REDUCE_AVERAGE ? s / (metric ? m : count) : s;
}

// the 64 lanes of a wave in a fixed tree; the result is valid in lane 0
template <int KIND> __device__ __forceinline__ double dg_wave_reduce(double x) {
    for (int w = 32; w > 0; w >>= 1) x = dg_combine<KIND>(x, __shfl_down(x, w, 64));
    return x;
}

struct DgRows {
    int n0, n1, n2;           // interior extents of the operand
    int rj, rk;               // y / z reduced
    int rows;                 // rows per output element: (rj ? n1 : 1) * (rk ? n2 : 1)
    int nch;                  // chunks per output element: ceil(rows / DG_ROWS)
    double count;             // points per output element
};

// x reduced. Block b: output element b / nch, chunk b % nch. slab: [0, nout * nch) the partial results, [nout * nch, 2 nout nch) the
// partial metric sums (average with a metric)
template <int KIND, class O, class W>
__global__ void __launch_bounds__(DG_THREADS) dg_reduce_rows_kernel(O o, DgRows R, W out, double *slab, long nslab) {
    __shared__ double lds[2][DG_THREADS / 64];
    const long b = blockIdx.x;
    const int e = (int)(b / R.nch), c = (int)(b % R.nch);
    const int ej = R.rj ? 1 : R.n1;
    const int jo = e % ej, ko = e / ej;                     // the kept (j, k) of the output element
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool with_metric = KIND == OCN_REDUCE_AVERAGE && o.mmode != 0;
    const int rend = min(R.rows, (c + 1) * DG_ROWS);
    double s = dg_identity<KIND>(), ms = 0.0;
    for (int r = c * DG_ROWS + wave; r < rend; r += DG_THREADS / 64) {
        const int jr = R.rj ? r % R.n1 : 0, kr = R.rk ? (R.rj ? r / R.n1 : r) : 0;
        const int j = jo + jr, k = ko + kr;
        for (int i = lane; i < R.n0; i += 64) {
            double m;
            s = dg_combine<KIND>(s, dg_eval(o, i, j, k, m));
            if (with_metric) ms = ms + m;
        }
    }
    s = dg_wave_reduce<KIND>(s);
    if (with_metric) ms = dg_wave_reduce<OCN_REDUCE_SUM>(ms);
    if (lane == 0) { lds[0][wave] = s; lds[1][wave] = ms; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < DG_THREADS / 64; ++w) {
        s = dg_combine<KIND>(s, lds[0][w]);
        if (with_metric) ms = ms + lds[1][w];
    }
    if (R.nch == 1) dg_store(out, out.off + jo * out.s[1] + ko * out.s[2], dg_finish<KIND>(s, ms, with_metric, R.count));
    else {
        slab[b] = s;
        if (with_metric) slab[nslab + b] = ms;
    }
}

// the chunks of one output element per block: thread t adds chunks t, t + 256, ... in order, the threads combine in a fixed tree
template <int KIND, class W>
__global__ void __launch_bounds__(DG_THREADS) dg_combine_kernel(DgRows R, W out, const double *slab, long nslab, int with_metric) {
    __shared__ double lds[2][DG_THREADS];
    const int e = blockIdx.x;
    const int ej = R.rj ? 1 : R.n1;
    const int jo = e % ej, ko = e / ej;
    double s = dg_identity<KIND>(), ms = 0.0;
    for (int c = threadIdx.x; c < R.nch; c += DG_THREADS) {
        s = dg_combine<KIND>(s, slab[(long)e * R.nch + c]);
        if (with_metric) ms = ms + slab[nslab + (long)e * R.nch + c];
    }
    lds[0][threadIdx.x] = s;
    lds[1][threadIdx.x] = ms;
    __syncthreads();
    for (int w = DG_THREADS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            lds[0][threadIdx.x] = dg_combine<KIND>(lds[0][threadIdx.x], lds[0][threadIdx.x + w]);
            lds[1][threadIdx.x] = lds[1][threadIdx.x] + lds[1][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) dg_store(out, out.off + jo * out.s[1] + ko * out.s[2], dg_finish<KIND>(lds[0][0], lds[1][0], with_metric != 0, R.count));
}

// x kept: thread (i, jo, ko) loops over the reduced y (inner) and z (outer) extents lj, lk (1 where the direction is kept)
template <int KIND, class O, class W>
__global__ void __launch_bounds__(256) dg_reduce_cols_kernel(O o, W out, int n0, int e1, int lj, int lk, double count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, jo = blockIdx.y * blockDim.y + threadIdx.y, ko = blockIdx.z;
    if (i >= n0 || jo >= e1) return;
    const bool with_metric = KIND == OCN_REDUCE_AVERAGE && o.mmode != 0;
    double s = dg_identity<KIND>(), ms = 0.0;
    for (int kr = 0; kr < lk; ++kr)
        for (int jr = 0; jr < lj; ++jr) {
            double m;
            s = dg_combine<KIND>(s, dg_eval(o, i, jo + jr, ko + kr, m));
            if (with_metric) ms = ms + m;
        }
    dg_store(out, out.off + i * out.s[0] + jo * out.s[1] + ko * out.s[2], dg_finish<KIND>(s, ms, with_metric, count));
}

// ---------------------------------------------------------------------------------------------------------------------
// accumulations: B[start] = A[start]; B[i] = B[i ∓ 1] + A[i] (accumulate_x / _y / _z, scans.jl:272-306)
// ---------------------------------------------------------------------------------------------------------------------
// along y (DIM 1) or z (DIM 2): thread (i, q), q the other of j, k; nd points along the march
// (a time average folds only what is stored: the running sum stays in registers)
template <int DIM, class O, class W>
__global__ void __launch_bounds__(256) dg_accumulate_cols_kernel(O o, W out, int n0, int nq, int nd, int reverse) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, q = blockIdx.y * blockDim.y + threadIdx.y;
    if (i >= n0 || q >= nq) return;
    double run = 0.0;
    for (int t = 0; t < nd; ++t) {
        const int d = reverse ? nd - 1 - t : t;
        const int j = DIM == 1 ? d : q, k = DIM == 1 ? q : d;
        double m;
        const double a = dg_eval(o, i, j, k, m);
        run = t == 0 ? a : run + a;
        dg_store(out, out.off + i * out.s[0] + j * out.s[1] + k * out.s[2], run);
    }
}

// along x: one wave per (j, k) row, 64 points per step; every lane forms the running sum of the step's values in index order
template <class O, class W>
__global__ void __launch_bounds__(DG_THREADS) dg_accumulate_rows_kernel(O o, W out, int n0, int n1, long nrows, int reverse) {
    const long row = (long)blockIdx.x * (DG_THREADS / 64) + (threadIdx.x >> 6);
    if (row >= nrows) return;                                // whole waves leave: the shuffles below see full waves
    const int lane = threadIdx.x & 63;
    const int j = (int)(row % n1), k = (int)(row / n1);
    double run = 0.0;
    for (int base = 0; base < n0; base += 64) {
        const int t = base + lane;                           // position along the march
        const int i = reverse ? n0 - 1 - t : t;
        double m, a = 0.0;
        if (t < n0) a = dg_eval(o, i, j, k, m);
        const int cnt = min(64, n0 - base);
        double mine = 0.0;
        for (int l = 0; l < cnt; ++l) {
            const double al = __shfl(a, l, 64);
            run = (base == 0 && l == 0) ? al : run + al;
            if (l == lane) mine = run;
        }
        if (t < n0) dg_store(out, out.off + i * out.s[0] + j * out.s[1] + k * out.s[2], mine);
    }
}
